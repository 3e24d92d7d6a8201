"""Watching the C ABI from Python: every status-returning entry point of gdn_amd._lib.lib (the ones that launch) is wrapped
while a function runs.  Shared by the tests (test_hip_partial_finetune, test_hip_engine_calls), the diagnostics under
tests/diag and the recorder tests/golden/gen_engine_calls.py."""
import collections
import ctypes


def watch_library_calls(fn, on_call):
    """Runs fn(); on_call(name, args) sees every launching library call first, in order."""
    from gdn_amd import _lib
    saved = {}
    for name in _lib._STATUS_FUNCS - {"gdn_conv_out_dims", "gdn_fftconv_cgemm_shape"}:      # (these two launch nothing)
        f = getattr(_lib.lib, name)
        saved[name] = f

        def watched(*a, _f=f, _n=name):
            on_call(_n, a)
            return _f(*a)
        setattr(_lib.lib, name, watched)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(_lib.lib, name, f)


def count_library_calls(fn):
    """Calls into the C ABI (status-returning entry points: the ones that launch) while fn() runs: (Counter by name, the
    names in call order)."""
    n, order = collections.Counter(), []

    def on_call(name, args):
        n[name] += 1
        order.append(name)
    watch_library_calls(fn, on_call)
    return n, order


def canonical_call(name, args):
    """[name, argument, ...] of one library call in a form that does not depend on addresses, by the argument types of
    _lib._SIGS: integers and floats by value, a gdn_conv_geom reference as the list of its eleven fields, every other
    pointer (the stream included) as 0 for null and 1 for non-null."""
    from gdn_amd import _lib
    types = _lib._SIGS[name][1]
    assert len(types) == len(args), (name, len(types), len(args))
    rec = [name]
    for t, a in zip(types, args):
        if t is _lib._PG:
            g = a._obj if hasattr(a, "_obj") else a.contents
            rec.append([int(getattr(g, f)) for f, _ in _lib.ConvGeom._fields_])
        elif t in (ctypes.c_float, ctypes.c_double):
            rec.append(float(a))
        elif t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint64):
            rec.append(int(a))
        else:                                          # c_void_p, POINTER(c_int32)
            rec.append(0 if a is None or (isinstance(a, int) and a == 0) else 1)
    return rec


def record_library_calls(fn):
    """canonical_call of every launching library call while fn() runs, in order."""
    out = []
    watch_library_calls(fn, lambda name, args: out.append(canonical_call(name, args)))
    return out
