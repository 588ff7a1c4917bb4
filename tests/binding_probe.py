"""CPU-only machinery that watches every pointer the Python package hands to the library (a helper like the `*_ref.py` files).

Three parts:

  header model   `header_model()` parses include/sslam_hip.h into {function: Proto(ret, [Param(name, cls, elem, const)])}.
                 cls is one of int / size_t / int64 / float / double / pointer / pointer-to-pointer; elem is float, double,
                 uint8_t, int8_t, int16_t, uint16_t, int32_t, int64_t, char, void or an opaque `sslam_*` handle type.
  tracked ptr    `Probe.ptr` replaces `_native.ptr` (the wrappers look it up at call time).  For every ndarray it records the
                 address, size, dtype, contiguity and a weak reference to the array that OWNS the memory (the end of the
                 `.base` chain: `K.reshape(9)` is a temporary view of a live `K` and is fine).  Ints are device addresses.
  ProbeLib       what a patched `_native.lib()` returns.  Every `sslam_*` attribute collects garbage, checks the pointer
                 arguments against the registry and the header (owner alive, C-contiguous, dtype of the parameter's element
                 type), converts every argument through the binding's own `argtypes` as ctypes would, copies the bytes of
                 the `const` arrays into the call record, writes a small reply (handles, capacities, counts) and returns 0.
                 The source of `sslam_memcpy_h2d_async` must still be alive at the next `sslam_ctx_sync` / `sslam_memcpy_d2h`
                 of the same context.

Nothing is raised inside a call: the findings collect in `Probe.reports` and the test asserts on them afterwards, so one run
names every site.  `install(monkeypatch)` installs all of it, with `_native.default_context` a `fake_device.FakeContext` that has
a `handle` and whose memory traffic goes through the (probed) library like the real `Context`'s."""
import ctypes as C
import gc
import re
import weakref
from collections import namedtuple

import numpy as np

import fake_device
from conftest import ROOT, load_pkg

Param = namedtuple("Param", "name cls elem const")
Proto = namedtuple("Proto", "ret params ret_elem")
Record = namedtuple("Record", "address nbytes dtype contiguous owner what")
Call = namedtuple("Call", "name args const_bytes")

_SCALARS = {"int": "int", "int32_t": "int", "size_t": "size_t", "int64_t": "int64", "float": "float", "double": "double"}
_ELEMS = {"int": "int32_t", "unsigned char": "uint8_t", "unsigned int": "uint32_t"}
# element type -> (numpy kinds, item size); void / char accept anything
_DTYPES = {"float": ("f", 4), "double": ("f", 8), "uint8_t": ("u", 1), "int8_t": ("i", 1), "int16_t": ("i", 2), "uint16_t": ("u", 2),
           "int32_t": ("i", 4), "uint32_t": ("u", 4), "int64_t": ("i", 8)}


def _parse_type(text):
    """'const float* pts1' -> (True, 1, ['float', 'pts1']); a return type has no name: 'const char*' -> (True, 1, ['char'])"""
    const = bool(re.search(r"\bconst\b", text))
    stars = text.count("*")
    words = re.sub(r"\bconst\b|\*", " ", text).split()
    return const, stars, words


def header_model(path=None):
    txt = (path or ROOT / "include" / "sslam_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = "\n".join(line for line in txt.splitlines() if not line.lstrip().startswith("#"))
    txt = re.sub(r'extern\s+"C"\s*\{', " ", txt)
    txt = re.sub(r"\btypedef\b[^;]*;", " ", txt)
    model = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(sslam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        const, stars, words = _parse_type(ret)
        base = " ".join(words)
        rcls = "pointer" if stars else _SCALARS[base]
        out = []
        if params.strip() != "void":
            for p in params.split(","):
                const, stars, words = _parse_type(p)
                pname, base = words[-1], " ".join(words[:-1])
                if stars == 0:
                    out.append(Param(pname, _SCALARS[base], None, False))
                else:
                    assert stars <= 2, (name, p)
                    out.append(Param(pname, "pointer" if stars == 1 else "pointer-to-pointer", _ELEMS.get(base, base), const))
        assert name not in model, f"{name} is declared twice"
        model[name] = Proto(rcls, out, _ELEMS.get(base, base) if stars else None)
    return model


def is_handle(p):
    return p.elem is not None and p.elem.startswith("sslam_")


def owner_of(a):
    """The object that owns the memory of ndarray `a`: the last ndarray of its `.base` chain, or the non-ndarray buffer that
    chain ends in."""
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a if a.base is None else a.base


class _Strong:
    """a reference to an object that takes no weak reference (bytes, memoryview): held, so alive"""

    def __init__(self, obj):
        self.obj = obj

    def __call__(self):
        return self.obj


DEVICE_BASE = 0x1000            # fake device addresses: far below any host mapping, 4 KiB apart


class Probe:
    def __init__(self, native, model=None):
        self.native = native
        self.model = model or header_model()
        self.signatures = native._signatures()
        self.registry = {}              # address -> Record of the LAST array `ptr` was given at that address
        self.reports = []
        self.calls = []
        self.reached = set()
        self.pending = {}               # context handle -> [Record] of asynchronous uploads not yet synchronised
        self._real_ptr = native.ptr
        self._next = DEVICE_BASE
        self._host_blocks = []
        self.replies = dict(REPLIES)
        self.lib = ProbeLib(self)

    # -- the tracked `_native.ptr` ------------------------------------------------------------------------------------------
    def ptr(self, a):
        if isinstance(a, np.ndarray):
            own = owner_of(a)
            try:
                ref = weakref.ref(own)
            except TypeError:
                ref = _Strong(own)
            addr = a.ctypes.data
            self.registry[addr] = Record(addr, a.nbytes, a.dtype, bool(a.flags["C_CONTIGUOUS"]), ref, f"{a.dtype} {a.shape}")
            return C.c_void_p(addr)             # (a non-contiguous array is reported at the call, with the function's name)
        if isinstance(a, int) and not isinstance(a, bool):
            self.registry[a] = Record(a, 0, None, True, None, "device")
        return self._real_ptr(a)

    def device_address(self, nbytes=0):
        p = self._next
        self._next += 0x1000 * (1 + int(nbytes) // 0x1000)
        return p

    def report(self, text):
        self.reports.append(text)

    def clear(self):
        self.reports.clear(); self.calls.clear(); self.pending.clear()

    def const_bytes(self, name=None):
        """[(function, parameter, bytes)] of every const array the library saw, in call order"""
        return [(c.name, k, v) for c in self.calls if name in (None, c.name) for k, v in c.const_bytes.items()]

    # -- one library call ---------------------------------------------------------------------------------------------------
    def _record_of(self, arg):
        if isinstance(arg, C.c_void_p) and arg.value is not None:
            return self.registry.get(arg.value)
        return None

    def call(self, name, args):
        gc.collect()
        self.reached.add(name)
        proto = self.model.get(name)
        if proto is None:
            self.report(f"{name}: not declared in the header")
            return 0
        if len(args) != len(proto.params):
            self.report(f"{name}: {len(args)} arguments, the header declares {len(proto.params)}")
            return 0
        argtypes = self.signatures[name][1]
        const_bytes, named = {}, {}
        for p, t, arg in zip(proto.params, argtypes, args):
            named[p.name] = arg
            try:
                t.from_param(arg)
            except (C.ArgumentError, TypeError, ValueError) as e:
                self.report(f"{name}: parameter {p.name}: ctypes refuses {type(arg).__name__} as {t.__name__} ({e})")
                continue
            if p.cls != "pointer" or is_handle(p):
                continue
            rec = self._record_of(arg)
            if rec is None or rec.dtype is None:
                continue
            alive = rec.owner() is not None
            if not alive:
                self.report(f"{name}: parameter {p.name}: the array that owns the memory ({rec.what}) was released before the call")
            if not rec.contiguous:
                self.report(f"{name}: parameter {p.name}: the array ({rec.what}) is not C-contiguous")
            want = _DTYPES.get(p.elem)
            if want is not None and (rec.dtype.kind not in want[0] or rec.dtype.itemsize != want[1]):
                self.report(f"{name}: parameter {p.name}: the array is {rec.dtype}, the header says {'const ' if p.const else ''}{p.elem}*")
            if p.const:
                const_bytes[p.name] = C.string_at(rec.address, rec.nbytes) if alive and rec.contiguous else None
        self.calls.append(Call(name, named, const_bytes))
        self._async(name, proto, named)
        ret = self._reply(name, proto, named)
        return ret

    def _async(self, name, proto, named):
        if name == "sslam_memcpy_h2d_async":
            rec = self._record_of(named["src_host"])
            if rec is not None and rec.dtype is not None:
                self.pending.setdefault(_value(named["ctx"]), []).append(rec)
        elif name in ("sslam_ctx_sync", "sslam_memcpy_d2h"):
            for rec in self.pending.pop(_value(named["ctx"]), []):
                if rec.owner() is None:
                    self.report(f"sslam_memcpy_h2d_async: parameter src_host: the array that owns the memory ({rec.what}) was released "
                                f"before {name} synchronised the upload")

    def _reply(self, name, proto, named):
        """defaults: a fresh handle / device address through every pointer-to-pointer, zeros through every other writable
        pointer; `self.replies[name]` = {parameter: value | callable(probe, named)} overrides, "return" sets the result"""
        over = self.replies.get(name, {})
        for p in proto.params:
            arg = named[p.name]
            if p.name in over:
                v = over[p.name]
                v = v(self, named) if callable(v) else v
            elif p.cls == "pointer-to-pointer":
                v = self.device_address()
            else:
                v = 0
            if not p.const and (p.cls == "pointer-to-pointer" or (p.cls == "pointer" and not is_handle(p))):
                self._write(arg, v)
        r = over.get("return", 0)
        return r(self, named) if callable(r) else r

    def _write(self, arg, v):
        obj = getattr(arg, "_obj", None)            # C.byref(x)
        if obj is not None:
            if hasattr(obj, "value"):
                obj.value = v
            return
        rec = self._record_of(arg)
        if rec is not None and rec.dtype is not None and rec.owner() is not None and rec.contiguous and rec.nbytes:
            if not isinstance(v, np.ndarray) and v == 0:
                C.memset(rec.address, 0, rec.nbytes)
            else:
                buf = np.frombuffer((C.c_uint8 * rec.nbytes).from_address(rec.address), rec.dtype)
                buf[:np.size(v) if isinstance(v, np.ndarray) else None] = v

    def host_block(self, nbytes):
        buf = (C.c_uint8 * max(int(nbytes), 1))()
        self._host_blocks.append(buf)
        return C.addressof(buf)


def _value(h):
    return h.value if isinstance(h, C.c_void_p) else h


class ProbeLib:
    def __init__(self, probe):
        self._probe = probe

    def __getattr__(self, name):
        if not name.startswith("sslam_"):
            raise AttributeError(name)
        probe = self._probe

        def entry(*args):
            return probe.call(name, args)
        entry.__name__ = name
        return entry


# what the wrappers need to carry on: capacities, counts and info words (everything else is a handle or zeros)
REPLIES = {
    "sslam_last_error": {"return": b""},
    "sslam_ctx_stream": {"return": None},
    "sslam_abi_version": {"return": 1},
    "sslam_device_count": {"n_out": 1},
    "sslam_malloc": {"dptr_out": lambda probe, a: probe.device_address(a["bytes"])},
    "sslam_host_alloc": {"hptr_out": lambda probe, a: probe.host_block(a["bytes"])},
    "sslam_orb_capacity": {"cap": 64},
    "sslam_sift_capacity": {"rows": 64, "candidates_or_null": 64},
    "sslam_akaze_capacity": {"rows": 64, "candidates_or_null": 64},
    "sslam_thumb_capacity": {"capacity": 4096},
    "sslam_lightglue_capacity": {"kc_out": 512},
    "sslam_orb_detect_host": {"n_out": 3},
    "sslam_sift_detect_host": {"n_out": 3},
    "sslam_akaze_detect_host": {"n_out": 3},
    "sslam_aliked_extract_host": {"n_out": 3},
    "sslam_thumb_encode_host": {"nbytes": 16},
    "sslam_orb_level_info": {"info8": 4},
    "sslam_sift_octave_info": {"info8": 4},
    "sslam_akaze_level_info": {"info12": 4},
    "sslam_klt_info": {"top_level": 1, "w": 8, "h": 6},
    "sslam_lightglue_match_host": {"k_out": 2, "stop_layer_out": 1},
    "sslam_lightglue_match_host_sized": {"k_out": 2, "stop_layer_out": 1},
    "sslam_bf_match_host": {"k_out": 2},
    "sslam_bf_ratio_match_host": {"k_out": 2},
}


class ProbeContext(fake_device.FakeContext):
    """`fake_device.FakeContext` with a `handle`; its memory traffic is the real `Context`'s code over the probed library, so the
    probe sees every upload and download a wrapper makes through its context."""

    def __init__(self, native, handle=0x7001):
        super().__init__()
        self.handle = C.c_void_p(handle)
        self.scratch, self._pinned = {}, []
        C_ = native.Context
        for m in ("sync", "malloc", "free", "h2d", "d2h", "host_alloc", "h2d_async", "d2h_async", "d2d_async", "memset_async", "event",
                  "timing_event", "record", "wait", "upload", "timer_start", "timer_stop"):
            setattr(self, m, getattr(C_, m).__get__(self))
        self.elapsed_ms = C_.elapsed_ms


def install(monkeypatch):
    """-> Probe, with `_native.ptr`, `_native.lib` and `_native.default_context` patched for the test's duration"""
    native = load_pkg("_native")
    probe = Probe(native)
    ctx = ProbeContext(native)
    monkeypatch.setattr(native, "ptr", probe.ptr)
    monkeypatch.setattr(native, "lib", lambda: probe.lib)
    monkeypatch.setattr(native, "default_context", lambda device=0: ctx)
    probe.ctx = ctx
    return probe
