"""C-ABI surface: the library builds, loads without a GPU, and exports every
symbol include/sslam_hip.h declares; the ctypes binding declares the same set."""
import re
from pathlib import Path

from conftest import ROOT, load_pkg


def _header_symbols():
    txt = (ROOT / "include" / "sslam_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sslam_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_symbols():
    syms = _header_symbols()
    assert "sslam_ctx_create" in syms and "sslam_ba_residual_jacobian_dev" in syms


def test_library_exports_every_declared_symbol():
    native = load_pkg("_native")
    lib = native.lib()
    for s in _header_symbols():
        assert hasattr(lib, s), f"libsslam_hip.so does not export {s}"


def _accepted(native, p):
    """the ctypes types that may stand for a header parameter (or a return type, whose name is empty)"""
    import ctypes as C
    scalar = {"int": C.c_int, "size_t": C.c_size_t, "int64": C.c_int64, "float": C.c_float, "double": C.c_double}
    if p.cls in scalar:
        return (scalar[p.cls],)
    if p.cls == "pointer-to-pointer":
        return (C.c_void_p, native.c_void_pp) if not p.const else (C.c_void_p,)
    if p.elem == "char":
        return (C.c_char_p,)
    return {"int32_t": (C.c_void_p, native.c_int_p), "float": (C.c_void_p, native.c_float_p)}.get(p.elem, (C.c_void_p,))


def test_binding_matches_header():
    import binding_probe
    native = load_pkg("_native")
    assert sorted(native.declared_symbols()) == _header_symbols()
    model, sigs = binding_probe.header_model(), native._signatures()
    assert sorted(model) == _header_symbols()
    for name, proto in model.items():
        res, args = sigs[name]
        ret = binding_probe.Param("", proto.ret, proto.ret_elem, True)
        assert res in _accepted(native, ret), f"{name}: returns {proto.ret} in the header, the binding says {res.__name__}"
        assert len(args) == len(proto.params), f"{name}: {len(proto.params)} parameters in the header, {len(args)} argtypes"
        for i, (p, t) in enumerate(zip(proto.params, args)):
            assert t in _accepted(native, p), (f"{name}: parameter {i} `{p.name}` is {p.cls}{' of ' + p.elem if p.elem else ''} in the header, "
                                               f"the binding says {t.__name__}")


def test_abi_version_and_error_string():
    native = load_pkg("_native")
    lib = native.lib()
    assert lib.sslam_abi_version() == 1
    # NULL out pointer -> error code + message, no crash, no GPU needed
    assert lib.sslam_device_count(None) != 0
    assert b"NULL" in lib.sslam_last_error()


def test_no_oracle_import_in_product():
    """The product path must never reach into oracle/ (tests-only checker)."""
    pkg_dir = ROOT / "opencv-simpleslam_amd"
    for p in pkg_dir.rglob("*.py"):
        src = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), p
