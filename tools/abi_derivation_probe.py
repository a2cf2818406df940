"""One-off: is the binding that gscream_amd/_native.py derives from include/gsraster.h the binding its hand-written tables were?

    git show <parent>:gscream_amd/_native.py > native_parent.py
    python tools/abi_derivation_probe.py native_parent.py

Loads the built library twice: through the given copy of the hand-written binding (pointed at the package's library by
GSR_LIB) and through the derivation (_abi.header + _abi.ctype with today's struct classes, which are compared by field list).
Prints every function whose restype or argtypes differ, position by position, the functions the old binding left untyped and what
they are now, and the constants whose values differ.  No GPU is needed.  profiles/abi_derivation.md holds the result."""
import ctypes
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import _abi, _native  # noqa: E402


def same(a, b):
    """ctypes types compare by identity, except POINTER(struct) of the two bindings' own classes: those by the structs' fields."""
    if a is b:
        return True
    if isinstance(a, type) and isinstance(b, type) and issubclass(a, ctypes._Pointer) and issubclass(b, ctypes._Pointer):
        fa, fb = a._type_._fields_, b._type_._fields_
        return len(fa) == len(fb) and all(x[0] == y[0] and same(x[1], y[1]) for x, y in zip(fa, fb))
    if isinstance(a, type) and isinstance(b, type) and issubclass(a, ctypes.Array) and issubclass(b, ctypes.Array):
        return a._length_ == b._length_ and a._type_ is b._type_
    return False


def main(parent_path):
    spec = importlib.util.spec_from_file_location("gscream_amd._native_parent", parent_path)
    old = importlib.util.module_from_spec(spec)
    os.environ.setdefault("GSR_LIB", _native.LIB_PATH)  # the copy lies outside the package: point it at the package's library
    spec.loader.exec_module(old)
    old_lib = old.load()
    abi = _abi.header()
    print(f"header: {len(abi.functions)} functions, {len(abi.constants)} constants, {len(abi.structs)} structs")
    print("symbol tuple equal (order included):", tuple(abi.functions) == tuple(old.EXPORTED_SYMBOLS),
          "| same set:", set(abi.functions) == set(old.EXPORTED_SYMBOLS))
    unset, bad_ret, bad_arg, n_ret, n_arg = [], [], [], 0, 0
    for name, (returns, params) in abi.functions.items():
        fn = getattr(old_lib, name)
        new_ret = _abi.ctype(returns, returns=True)
        new_args = [_abi.ctype(c, _native.STRUCTS) for c, _, _, _ in params]
        n_ret += 1
        if fn.restype is not new_ret:
            bad_ret.append((name, fn.restype, new_ret))
        if fn.argtypes is None:
            unset.append((name, new_args))
            continue
        n_arg += 1
        if len(fn.argtypes) != len(new_args) or not all(same(a, b) for a, b in zip(fn.argtypes, new_args)):
            bad_arg.append((name, list(fn.argtypes), new_args))
    print(f"restype compared: {n_ret}, different: {len(bad_ret)}")
    for row in bad_ret:
        print("   ", *row)
    print(f"argtypes compared: {n_arg}, different: {len(bad_arg)}")
    for row in bad_arg:
        print("   ", *row)
    print(f"argtypes unset in the hand-written binding: {len(unset)}")
    for name, args in unset:
        print(f"    {name}: None -> {args}")
    names = [n for n in dir(old) if n.isupper() and isinstance(getattr(old, n), (int, tuple)) and n not in ("EXPORTED_SYMBOLS",)]
    diff = [(n, getattr(old, n), getattr(_native, n, "<gone>")) for n in names if getattr(old, n) != getattr(_native, n, "<gone>")]
    print(f"constants compared: {len(names)} ({' '.join(names)}), different: {len(diff)}")
    for row in diff:
        print("   ", *row)
    return 1 if bad_ret or bad_arg or diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
