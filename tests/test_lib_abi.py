"""CPU-side checks of the C ABI: the shared library builds/loads here (no GPU needed) and
exports every function include/dmp_hip.h declares; the ctypes table mirrors the header."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "dmp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dmp_[a-z0-9_]+)\s*\(", text)))


def test_header_functions_are_exported_and_bound():
    from dualmessagepassing_amd import _build, _lib
    path = _build.build_lib()
    lib = ctypes.CDLL(path)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libdmp_hip.so does not export " + n
        assert n in _lib.SIGNATURES, "ctypes table lacks " + n
    assert sorted(_lib.SIGNATURES) == names


def _header():
    import util_header
    return util_header.read(os.path.join(ROOT, "include", "dmp_hip.h"))


def _struct_classes(abi):
    return {n: c for n, c in vars(abi).items() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}


def test_header_reader_reads_the_whole_header_and_refuses_what_it_does_not_know():
    """The reader behind the checks below: it finds every function the name scan finds (at least the 159 functions and 22
    structs of ABI 90), and a declaration it cannot read is an error, not a skipped line."""
    import util_header
    import pytest
    h = _header()
    assert sorted(h.functions) == _declared()
    assert len(h.functions) >= 159 and len(h.structs) >= 22
    assert h.defines["DMP_ABI_VERSION"] >= 90
    wrap = 'extern "C" {\n%s\n}\n'
    ok = util_header.Header(wrap % "typedef struct { const float *a, *b; int n; } dmp_t;\nint dmp_f(const dmp_t *t, int64_t n);")
    assert ok.structs["dmp_t"] == [("a", "float", True, None), ("b", "float", True, None), ("n", "int", False, None)]
    assert ok.functions["dmp_f"] == (("int", False), [("t", "dmp_t", True), ("n", "int64_t", False)])
    for bad in ("int dmp_f(long n);", "int dmp_f(const dmp_t *t);", "typedef struct { short n; } dmp_t;", "int dmp_f(int64_t);",
                "typedef struct { int a[DMP_N]; } dmp_t;", "int dmp_f(int n)", "int dmp_f(int (*cb)(int));", "int dmp_f(int n); // x"):
        with pytest.raises(util_header.HeaderError):
            util_header.Header(wrap % bad)


def test_every_signature_equals_the_header():
    """Return type and the whole argument list of every declared function: count, order, and per argument the header's C
    type as ctypes (a data pointer: c_void_p; ``const dmp_X *``: POINTER(dmp_X); scalars by their exact type)."""
    from dualmessagepassing_amd import _abi
    h = _header()
    assert sorted(_abi.SIGNATURES) == sorted(h.functions)
    wrong = []
    for name in h.functions:
        res, args = h.signature(_abi, name)
        got_res, got_args = _abi.SIGNATURES[name]
        if got_res is not res:
            wrong.append("%s returns %s, the header says %s" % (name, got_res, res))
        if len(got_args) != len(args):
            wrong.append("%s takes %d arguments, the header says %d" % (name, len(got_args), len(args)))
            continue
        for i, (g, w) in enumerate(zip(got_args, args)):
            if g is not w:
                wrong.append("%s argument %d (%s) is %s, the header says %s" % (name, i, h.functions[name][1][i][0], g, w))
    assert not wrong, "\n".join(wrong)


def test_every_struct_equals_the_header():
    """A class per ``typedef struct`` of the header, under its name, with the header's fields in the header's order and types
    (arrays with the length of their ``#define``), and no other struct class.  Equal fields are equal layouts: ctypes lays a
    Structure without ``_pack_`` out by the platform's C rules."""
    from dualmessagepassing_amd import _abi
    h = _header()
    classes = _struct_classes(_abi)
    assert sorted(classes) == sorted(h.structs)
    for name, cls in classes.items():
        assert cls.__name__ == name
        assert "_pack_" not in vars(cls) and not getattr(cls, "_pack_", 0), name + " sets _pack_"
        assert [(f, t) for f, t, *_ in cls._fields_] == h.fields(_abi, name), name


def test_every_exported_limit_equals_the_header():
    from dualmessagepassing_amd import _abi
    h = _header()
    limits = {n: v for n, v in vars(_abi).items() if n.startswith("DMP_")}
    assert limits, "the binding exports no limit"
    for n, v in limits.items():
        assert n in h.defines, n + " is no #define of the header"
        assert v == h.defines[n], "%s = %r, the header says %r" % (n, v, h.defines[n])
    assert _abi.ABI_VERSION == h.defines["DMP_ABI_VERSION"]


def test_fold_field_walks_are_the_structs_fields():
    """``fused._FoldLayers`` fills the four fold blocks by walking these tuples: each is exactly its struct's fields, in order."""
    from dualmessagepassing_amd import _abi, fused

    def names(cls):
        return [f for f, *_ in cls._fields_]
    assert list(fused._FOLD_IN + fused._FOLD_AUX_IN) == names(_abi.dmp_layer_weights)
    assert list(fused._FOLD_OUT + fused._FOLD_AUX_OUT) == names(_abi.dmp_layer_folded)
    assert ["d" + f for f in fused._FOLD_OUT] == names(_abi.dmp_layer_folded_grads)
    assert list(fused._FOLD_GRAD) == names(_abi.dmp_layer_weight_grads)


def test_struct_arguments_refuse_other_objects_on_the_host():
    """A ``const dmp_X *`` parameter takes an array of dmp_X, ``byref`` of one or None; another struct's array or a bare
    address is an ArgumentError from ctypes -- raised while converting the arguments, so the library is never entered."""
    import pytest
    from dualmessagepassing_amd import _abi, _lib
    lib = _lib.load()
    assert lib.dmp_collate_jobs.argtypes[0] is ctypes.POINTER(_abi.dmp_collate_job)
    for wrong in ((_abi.dmp_pool_job * 1)(), ctypes.byref(_abi.dmp_pool_job()), 4096, "jobs"):
        with pytest.raises(ctypes.ArgumentError):
            lib.dmp_collate_jobs(wrong, 1, None)


def test_abi_version_and_workspace_queries():
    from dualmessagepassing_amd import _lib
    lib = _lib.load()
    assert lib.dmp_abi_version() == _lib.ABI_VERSION
    assert lib.dmp_csr_workspace_words(1000, 5000) >= 1000
    assert lib.dmp_scan_workspace_words(5000) >= 3
    w = lib.dmp_dedupe_table_words(1000)
    assert w >= 2000 and (w & (w - 1)) == 0


def test_loaded_library_matches_the_shipped_sources():
    """The library the suite runs is the one the sources in this tree build: content hash equal, ABI number equal to the
    header's (nothing asserted it; a stale library after a failed build passed silently)."""
    from dualmessagepassing_amd import _build, _lib
    lib = _lib.load()
    assert not _build._stale(), "csrc/libdmp_hip.so was not built from the sources in this tree"
    hdr = open(os.path.join(ROOT, "include", "dmp_hip.h")).read()
    assert lib.dmp_abi_version() == int(re.search(r"#define\s+DMP_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_stale_library_after_a_failed_build_is_refused(monkeypatch):
    """``_lib.load``: a failed build + a library whose hash does not match the sources -> DmpError (not a line on stderr);
    DMP_ALLOW_STALE_LIB=1 is the explicit way around; a failed build beside a CURRENT library still loads it."""
    import pytest
    from dualmessagepassing_amd import _build, _lib

    def boom(*a, **k):
        raise RuntimeError("hipcc failed on dmp_typed.hip:\nerror: pretend")

    monkeypatch.setattr(_build, "build_lib", boom)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_build, "_stale", lambda: True)
    monkeypatch.delenv("DMP_ALLOW_STALE_LIB", raising=False)
    with pytest.raises(_lib.DmpError, match="STALE"):
        _lib.load()
    monkeypatch.setenv("DMP_ALLOW_STALE_LIB", "1")
    assert _lib.load() is not None
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.delenv("DMP_ALLOW_STALE_LIB", raising=False)
    monkeypatch.setattr(_build, "_stale", lambda: False)
    assert _lib.load() is not None


def test_launch_timer_leaves_out_stalled_launches_only():
    """``_lib.uninterrupted`` (the per-launch timer behind bench.py's roofline objects): a launch stalled by the box (20 ms among
    27 us ones) is left out; a kernel's own spread -- twice, five times the median, or 10x a sub-100-us median without the extra
    millisecond -- is not."""
    from dualmessagepassing_amd import _lib
    base = [0.027] * 30 + [0.031] * 29
    assert _lib.uninterrupted(base + [20.4]) == base
    assert _lib.uninterrupted(base + [0.135]) == base + [0.135]
    assert _lib.uninterrupted(base + [0.9]) == base + [0.9]          # > 10x the median but < 1 ms above it: kept
    assert _lib.uninterrupted([5.0, 5.0, 49.0]) == [5.0, 5.0, 49.0]  # < 10x
    assert _lib.uninterrupted([3.0]) == [3.0]
