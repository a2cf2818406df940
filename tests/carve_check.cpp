// carve_check.cpp -- GsrCarver on its own, as a host program (tests/test_workspace_sizes.py builds it with
// -fsanitize=address,undefined and runs it): every piece on its alignment, pieces in order and apart, the null-base walk with the
// same total and no pointer, an alias + skip pair as large as its larger user, a wrapping count caught; and the record of named
// pieces: every offset = pointer - base, the null-base walk records the same table, an alias + skip pair lists both users at one
// offset, unnamed pieces are left out, a short record array is counted past and not overrun.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../gscream_amd/csrc/gsr_carve.h"

#define CHECK(c) do { if (!(c)) { printf("carve_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct Piece { size_t count, size, align; };
template <size_t S> struct Bytes { char b[S]; };

// take() of `count` elements of `size` bytes
static char* take(GsrCarver& c, const Piece& p)
{
    switch (p.size) {
    case 1: return (char*)c.take<Bytes<1>>(p.count, p.align);
    case 4: return (char*)c.take<Bytes<4>>(p.count, p.align);
    case 8: return (char*)c.take<Bytes<8>>(p.count, p.align);
    case 12: return (char*)c.take<Bytes<12>>(p.count, p.align);
    case 64: return (char*)c.take<Bytes<64>>(p.count, p.align);
    }
    CHECK(!"size");
    return nullptr;
}

static void check_run(const Piece* run, int n)
{
    GsrCarver query(nullptr);
    for (int i = 0; i < n; i++) CHECK(take(query, run[i]) == nullptr);
    CHECK(query.ok() && query.total() == query.bytes());

    char* base = (char*)aligned_alloc(512, query.bytes() ? (query.bytes() + 511) / 512 * 512 : 512);
    CHECK(base);
    GsrCarver c(base);
    char* end = base;  // where the previous piece ended
    for (int i = 0; i < n; i++) {
        const size_t at = c.bytes();
        char* p = take(c, run[i]);
        const size_t used = run[i].count * run[i].size;
        CHECK(p == base + at && p >= end);
        CHECK(c.bytes() - at >= used && c.bytes() - at < used + run[i].align && (c.bytes() - at) % run[i].align == 0);
        // a run on ONE alignment keeps every piece on it (mixed runs start a piece where the previous one ended)
        bool uniform = true;
        for (int k = 0; k < i; k++) uniform = uniform && run[k].align == run[i].align;
        if (uniform) CHECK((size_t)(p - base) % run[i].align == 0);
        if (used) memset(p, 0xa5, used);  // inside the allocation, or AddressSanitizer says so
        end = p + used;
    }
    CHECK(c.ok() && c.bytes() == query.bytes() && end <= base + c.bytes());
    free(base);
}

int main()
{
    const Piece r256[] = {{1, 64, 256}, {1, 8, 256}, {63, 4, 256}, {64, 4, 256}, {65, 4, 256}, {0, 8, 256}, {2049, 1, 256}, {100000, 12, 256}};
    const Piece r512[] = {{3 * 17 * 33, 4, 512}, {5, 8, 512}, {128, 4, 512}, {129, 4, 512}};
    const Piece r16[] = {{17, 1, 16}, {5, 12, 16}, {3, 4, 16}, {16, 1, 16}, {0, 4, 16}, {1, 1, 16}};
    const Piece packed[] = {{24, 8, 8}, {7, 8, 8}};
    const Piece mixed[] = {{5, 1, 16}, {1, 64, 256}, {3, 4, 16}};
    check_run(r256, 8);
    check_run(r512, 4);
    check_run(r16, 6);
    check_run(packed, 2);
    check_run(mixed, 3);
    check_run(r256, 0);

    // two users of one area: the pair reserves the larger, whichever it is
    const size_t users[][2] = {{2592, 5120}, {5120, 2592}, {256, 256}, {0, 1}};
    for (const auto& u : users) {
        alignas(256) static char area[8192];
        GsrCarver c(area), q(nullptr);
        CHECK(c.take<uint32_t>(10) == (uint32_t*)area);
        float* a = c.alias<float>();
        uint32_t* b = c.alias<uint32_t>();
        CHECK((char*)a == area + 256 && (char*)b == area + 256 && c.bytes() == 256);
        const size_t larger = u[0] > u[1] ? u[0] : u[1];
        c.skip(larger);
        char* next = c.take<char>(1);
        CHECK(next >= (char*)a + u[0] && next >= (char*)b + u[1] && next == area + 256 + (larger + 255) / 256 * 256);
        (void)q.take<uint32_t>(10);
        CHECK(q.alias<float>() == nullptr);
        q.skip(larger);
        CHECK(q.take<char>(1) == nullptr && q.bytes() == c.bytes());
    }

    // a product or a sum that wraps: flagged, and it stays flagged; a size query then answers 0
    {
        GsrCarver c(nullptr);
        (void)c.take<Bytes<64>>(1);
        CHECK(c.ok() && c.total() == 256);
        (void)c.take<Bytes<64>>((size_t)-1 / 32);  // count * 64 wraps
        CHECK(!c.ok() && c.total() == 0);
        (void)c.take<char>(1);
        CHECK(!c.ok());
        GsrCarver d(nullptr);
        (void)d.take<char>((size_t)-1 - 300);  // fits
        CHECK(d.ok());
        (void)d.take<char>(1024);              // the running sum wraps
        CHECK(!d.ok() && d.total() == 0);
        GsrCarver e(nullptr);
        e.skip((size_t)-1 - 100);              // the rounding itself wraps
        CHECK(!e.ok());
    }
    // the record: a walk on a workspace and the same walk on a null base note the same table, each offset = pointer - base
    {
        auto walk = [](GsrCarver& c, char** at) {
            at[0] = (char*)c.take<Bytes<64>>("rec", 3);
            (void)c.take<uint32_t>(5);  // unnamed: cut, not recorded
            at[1] = (char*)c.take<Bytes<8>>("rect", 65);
            at[2] = (char*)c.alias<float>("ckpt", 648);
            at[3] = (char*)c.alias<uint32_t>("occ_mass", 1280);
            c.skip(5120);
            at[4] = (char*)c.take<uint8_t>("flags", 0);
            at[5] = (char*)c.take<Bytes<12>>("tail", 7, 16);
        };
        const char* names[] = {"rec", "rect", "ckpt", "occ_mass", "flags", "tail"};
        const size_t counts[] = {3, 65, 648, 1280, 0, 7}, sizes[] = {64, 8, 4, 4, 1, 12};
        alignas(256) static char area[8192];
        gsr_layout_piece with_base[6], without[6];
        GsrCarveRecord ra = {with_base, 6, 0}, rq = {without, 6, 0};
        GsrCarver c(area, &ra), q(nullptr, &rq);
        char *at[6], *none[6];
        walk(c, at);
        walk(q, none);
        CHECK(ra.count == 6 && rq.count == 6 && c.bytes() == q.bytes() && c.bytes() <= sizeof area);
        for (int i = 0; i < 6; i++) {
            CHECK(none[i] == nullptr && with_base[i].offset == (size_t)(at[i] - area) && without[i].offset == with_base[i].offset);
            CHECK(!strcmp(with_base[i].name, names[i]) && !strcmp(without[i].name, names[i]));
            CHECK(with_base[i].count == counts[i] && without[i].count == counts[i]);
            CHECK(with_base[i].elem_size == sizes[i] && without[i].elem_size == sizes[i]);
        }
        CHECK(with_base[2].offset == with_base[3].offset && with_base[4].offset == with_base[2].offset + 5120);
        // the same walk without a record leaves the same pointers
        GsrCarver plain(area);
        char* again[6];
        walk(plain, again);
        for (int i = 0; i < 6; i++) CHECK(again[i] == at[i]);
        CHECK(plain.bytes() == c.bytes());
        // a record array of two (heap: AddressSanitizer watches its end), then of none: filled as far as it goes, all six counted
        gsr_layout_piece* two = (gsr_layout_piece*)malloc(2 * sizeof(gsr_layout_piece));
        CHECK(two);
        GsrCarveRecord rs = {two, 2, 0}, r0 = {nullptr, 0, 0};
        GsrCarver s(nullptr, &rs), z(nullptr, &r0);
        walk(s, none);
        walk(z, none);
        CHECK(rs.count == 6 && r0.count == 6 && !strcmp(two[1].name, "rect") && two[1].offset == with_base[1].offset);
        free(two);
    }
    printf("carve_check OK\n");
    return 0;
}
