// gsr_carve.h -- the one walk that cuts a caller-allocated workspace into arrays.  Every workspace layout of the library is ONE function
// written on GsrCarver: the launcher runs it on the caller's pointer, the *_bytes query runs the same function on a null base and returns
// total(), so the two cannot disagree.  Host-only and free of HIP: a plain C++17 compiler takes it (tests/carve_check.cpp).
//
// A piece starts at the running total and advances it by count * sizeof(T) rounded up to `align` (256 for device arrays, 512 in lpips,
// 16 in the png / jpeg byte layouts, 8 where partial sums are packed).  The start itself is not aligned separately: a workspace whose
// base and pieces all use one `align` keeps every piece on it.
// With a null base no pointer is formed -- take() and alias() return nullptr -- so a size query does no arithmetic on a null pointer.
//
// The walk can also say what it cut: a carver given a GsrCarveRecord notes every NAMED piece there (name, offset, count, element size),
// with a null base as well, so a layout query is the same walk again.  Unnamed pieces and a carver without a record cost one null check.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/gsraster.h"  // gsr_layout_piece: what a record holds is what gsr_workspace_layout hands out

// caller-owned: pieces[capacity]; `count` = named pieces met, which may exceed capacity (the ones beyond it are counted, not written)
struct GsrCarveRecord { gsr_layout_piece* pieces; int capacity; int count; };

struct GsrCarver {
    explicit GsrCarver(void* base, GsrCarveRecord* record = nullptr) : base_(static_cast<char*>(base)), record_(record) {}
    // the next `count` T's
    template <class T> T* take(size_t count, size_t align = 256) { return take<T>(nullptr, count, align); }
    // ... under a name, for the record
    template <class T> T* take(const char* name, size_t count, size_t align = 256)
    {
        T* p = alias<T>(name, count);
        size_t n;
        if (__builtin_mul_overflow(count, sizeof(T), &n)) ok_ = false;
        skip(n, align);
        return p;
    }
    // the current position, no advance: a second user (of `count` T's, for the record) of the area the next take() / skip() reserves
    template <class T> T* alias(const char* name = nullptr, size_t count = 0) const
    {
        if (record_ && name) {
            if (record_->count < record_->capacity) record_->pieces[record_->count] = { name, off_, count, sizeof(T) };
            record_->count++;
        }
        return base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    }
    // advance past `bytes` (an aliased area, or a workspace embedded whole)
    void skip(size_t bytes, size_t align = 256)
    {
        size_t padded;
        if (__builtin_add_overflow(bytes, align - 1, &padded) || __builtin_add_overflow(off_, padded & ~(align - 1), &off_)) ok_ = false;
    }
    size_t bytes() const { return off_; }             // total so far = offset of the next piece
    bool ok() const { return ok_; }                   // no product or sum has wrapped
    size_t total() const { return ok_ ? off_ : 0; }   // what a size query returns: 0 = rejected, as for every size out of range

private:
    char* base_;
    GsrCarveRecord* record_;
    size_t off_ = 0;
    bool ok_ = true;
};
