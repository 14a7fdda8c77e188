"""ctypes binding of libhtk_amd.so (the C ABI of include/htk_amd.h) plus thin Python holders.

This is the host-side mirror used by the tests, bench.py and the Python drivers.  It contains no
numerics: every score, trellis and statistic comes from the HIP kernels behind the C ABI, and the
import fails loudly when the shared object is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "libhtk_amd.so")

LZERO = -1.0e10
LSMALL = -0.5e10
NOPRUNE = 1.0e20
UPMEANS, UPVARS, UPTRANS, UPMIXES = 1, 2, 4, 8
UPALL = 15
UPMAP = 32
UTT_OK, UTT_SKIPPED, UTT_ETEE, UTT_EALPHA = 1, 0, -7332, -7390


def _stream(s):
    """A stream or device address from outside (torch: stream.cuda_stream, tensor.data_ptr(); a c_void_p; None) as a void * parameter takes it."""
    return s if s is None or isinstance(s, C.c_void_p) else int(s)


SCORE_EXACT, SCORE_MFMA, SCORE_FASTLADD, SCORE_BF16, SCORE_SOUTP, SCORE_DIAGC, SCORE_F16 = 0, 1, 2, 4, 8, 16, 32
ERANGE = -7
COMPAT_STREAM_REVISIT = 1
COMPAT_SHARED_LOGWT = 2
ORDER_AUTO, ORDER_FAST, ORDER_EXACT = 0, 1, 2


class HtkAmdError(RuntimeError):
    rc = 0


class ModelDesc(C.Structure):
    _fields_ = [("vecSize", C.c_int), ("numStates", C.c_int), ("numComp", C.c_int), ("numGauss", C.c_int),
                ("numTrans", C.c_int), ("numPhys", C.c_int),
                ("stateCompOff", C.c_void_p), ("compWeight", C.c_void_p), ("compGauss", C.c_void_p),
                ("mean", C.c_void_p), ("var", C.c_void_p), ("gconst", C.c_void_p),
                ("transN", C.c_void_p), ("transOff", C.c_void_p), ("transP", C.c_void_p),
                ("hmmTrans", C.c_void_p), ("hmmStateOff", C.c_void_p), ("hmmState", C.c_void_p),
                ("numStreams", C.c_int), ("dimStream", C.c_void_p), ("hsKind", C.c_int), ("streamWeight", C.c_void_p)]


class AccsLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("mu", "muOcc", "va", "vaOcc", "wt", "wtOcc", "tr", "trOcc", "nEgs",
                                         "totalPr", "totalT", "nUttDone", "nUttSkipped", "nEval", "total")]


class FbConfig(C.Structure):
    _fields_ = [("pruneInit", C.c_double), ("pruneInc", C.c_double), ("pruneLim", C.c_double),
                ("minFrwdP", C.c_float), ("uFlags", C.c_int), ("scoreMode", C.c_int)]


class UpdateConfig(C.Structure):
    _fields_ = [("minEgs", C.c_int), ("minVar", C.c_float), ("mixWeightFloor", C.c_float), ("uFlags", C.c_int),
                ("singleProcess", C.c_int), ("varFloor", C.POINTER(C.c_float)), ("rowNormalise", C.c_int), ("mapTau", C.c_float), ("mapMinObs", C.c_float)]


class UpdateStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nFloorVar", "nFloorVarMix", "nSkippedHmm", "nNoTransOut", "nNoMixUse", "nNoVarUse", "nWeightAboveOne", "nMapObserved")]


class BatchDesc(C.Structure):
    _fields_ = [("nUtt", C.c_int), ("dX", C.c_void_p), ("frameOff", C.c_void_p), ("labOff", C.c_void_p), ("labs", C.c_void_p)]


_lib = None


def lib():
    """Load the native library.  There is deliberately no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise HtkAmdError("%s is missing: run `python -m htk_amd.build` (hipcc --offload-arch=gfx950)" % LIBPATH)
        L = C.CDLL(LIBPATH)
        abi.declare(L, STRUCTS)      # every prototype of include/htk_amd.h, once: a wrong argument is a TypeError at the call
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        e = HtkAmdError("%s failed (%d): %s" % (what, rc, lib().htkamd_last_error().decode()))
        e.rc = rc
        raise e


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Handle:
    """The owner of one C handle `h`: close() gives it to the class's destroy function once, and so does the finaliser."""
    _destroy = None

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevArray:
    """A device buffer owned through the C ABI (hipMalloc)."""

    def __init__(self, host: np.ndarray | None = None, nbytes: int | None = None):
        self.ptr = C.c_void_p()
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        check(lib().htkamd_dev_malloc(C.byref(self.ptr), self.nbytes), "dev_malloc")
        if host is not None:
            h = np.ascontiguousarray(host)
            check(lib().htkamd_memcpy_h2d(self.ptr, _p(h), h.nbytes, None), "memcpy_h2d")

    def to_host(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().htkamd_memcpy_d2h(_p(out), self.ptr, out.nbytes, None), "memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            lib().htkamd_dev_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def offsets(lengths) -> np.ndarray:
    """The int32 exclusive prefix sum of `lengths` -- frameOff, labOff, sampOff of a batch --, [0] for no lengths."""
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _pack(arrays, dtype, cols=None, who="batch"):
    """(host, off): the arrays one behind the other as ONE C-contiguous `dtype` array, and offsets() of their lengths.  Every array has the
    same shape behind its first axis: (cols,) where cols is given, else the first array's (vectors give a vector).  No array at all gives
    [0, cols], or an empty vector.  An array of another shape is an HtkAmdError in `who`'s name."""
    arrays = [np.asarray(a, dtype) for a in arrays]
    tail = (cols,) if cols is not None else arrays[0].shape[1:] if arrays else ()
    for u, a in enumerate(arrays):
        if a.ndim == 0 or a.shape[1:] != tail:
            raise HtkAmdError("%s: array %d of the batch has shape %s, %s expected" % (who, u, a.shape, ("n",) + tail))
    host = np.concatenate(arrays) if arrays else np.zeros((0,) + tail, dtype)
    return host, offsets([len(a) for a in arrays])


class _Batch:
    """A list of per-utterance arrays as the C ABI takes a batch: `host` and `off` (_pack), `n` arrays, and `dev`, the DevArray of `host`.
    The empty batch: without a single row `dev` is still a device buffer, of 4 bytes, so no entry point is handed a null table.  The holder
    owns all of them, and the C calls read `off` and `dev`: it lives until its call has returned and the results are unpacked."""

    def __init__(self, arrays, dtype, cols=None, who="batch"):
        self.host, self.off = _pack(arrays, dtype, cols, who)
        self.n = len(self.off) - 1
        self.dev = DevArray(self.host) if self.host.size else DevArray(nbytes=4)


def _desc_from_packed(pk: dict):
    """(ModelDesc, keepalive) from a packed dict -- for the pure-host entry points that take a description."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    k = dict(stateCompOff=i32(pk["stateCompOff"]), compWeight=f32(pk["compWeight"]), compGauss=i32(pk["compGauss"]),
             mean=f32(pk["mean"]), var=f32(pk["var"]), gconst=f32(pk.get("gconst")),
             transN=i32(pk["transN"]), transOff=i32(pk["transOff"]), transP=f32(pk["transP"]),
             hmmTrans=i32(pk["hmmTrans"]), hmmStateOff=i32(pk["hmmStateOff"]), hmmState=i32(pk["hmmState"]),
             dimStream=i32(pk["dimStream"]) if pk.get("dimStream") is not None else None, streamWeight=f32(pk.get("streamWeight")))
    d = ModelDesc(int(pk["vecSize"]), int(pk["numStates"]), int(pk["numComp"]), int(pk["numGauss"]), int(pk["numTrans"]), int(pk["numPhys"]),
                  _p(k["stateCompOff"]), _p(k["compWeight"]), _p(k["compGauss"]), _p(k["mean"]), _p(k["var"]), _p(k["gconst"]),
                  _p(k["transN"]), _p(k["transOff"]), _p(k["transP"]), _p(k["hmmTrans"]), _p(k["hmmStateOff"]), _p(k["hmmState"]),
                  int(pk.get("numStreams", 1) or 1), _p(k["dimStream"]), int(pk.get("hsKind", 0) or 0), _p(k["streamWeight"]))
    return d, k


class Model(_Handle):
    """htkamd_model holder.  `pk` is the packed layout dict (htk_amd.synth.SynthSet.packed() / the MMF loader)."""
    _destroy = "htkamd_model_destroy"

    def __init__(self, pk: dict):
        self.pk = pk
        d, k = _desc_from_packed(pk)
        self._keep = k
        self.NS = d.numStreams
        self.h = C.c_void_p()
        self.full = pk.get("invCov") is not None
        if self.full:       # FULLC set: the packed inverse-covariance triangles, desc.var unused (htkamd_model_create_full)
            k["invCov"] = np.ascontiguousarray(pk["invCov"], np.float32).reshape(-1)
            check(lib().htkamd_model_create_full(C.byref(d), _p(k["invCov"]), C.byref(self.h)), "model_create_full")
        else:
            check(lib().htkamd_model_create(C.byref(d), C.byref(self.h)), "model_create")
        self.D, self.S, self.C, self.G = d.vecSize, d.numStates, d.numComp, d.numGauss
        self.nT, self.H = d.numTrans, d.numPhys
        self.maxN = int(np.max(k["transN"]))

    def set_sharing(self, meanShare, varShare):
        """Tied mean / variance vectors (htkamd_model_set_sharing): arrays [G] of share numbers, -1 = private."""
        ms = np.ascontiguousarray(meanShare, np.int32); vs = np.ascontiguousarray(varShare, np.int32)
        check(lib().htkamd_model_set_sharing(self.h, _p(ms), _p(vs)), "model_set_sharing")

    def set_compat(self, flags: int):
        """The reference's own arithmetic where the library computes something else (htkamd_model_set_compat; COMPAT_STREAM_REVISIT)."""
        check(lib().htkamd_model_set_compat(self.h, int(flags)), "model_set_compat")

    def set_scan_order(self, order):
        """The order in which UpdateModels visits the physical models (htkamd_model_set_scan_order; hmm_scan_order() gives HTK's)."""
        o = np.ascontiguousarray(order, np.int32)
        assert o.shape == (self.H,)
        check(lib().htkamd_model_set_scan_order(self.h, _p(o)), "model_set_scan_order")

    def set_params(self, mean=None, var=None, gconst=None, compWeight=None, transP=None):
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        args = [f32(mean), f32(var), f32(gconst), f32(compWeight), f32(transP)]
        check(lib().htkamd_model_set_params(self.h, *[_p(a) for a in args]), "model_set_params")

    def get_prepared(self):
        ivar = np.empty((self.G, self.D), np.float32); gc = np.empty(self.G, np.float32)
        lw = np.empty(self.C, np.float32); md = np.empty(self.nT, np.int32)
        check(lib().htkamd_model_get_prepared(self.h, _p(ivar), _p(gc), _p(lw), _p(md)), "model_get_prepared")
        return dict(ivar=ivar, gconst=gc, compLogWt=lw, minDur=md)

    def _update_config(self, minEgs, minVar, mixWeightFloor, uFlags, singleProcess, varFloor, rowNormalise, mapTau=0.0, mapMinObs=0.0):
        """(htkamd_update_config, the array its varFloor points into)"""
        vf = None if varFloor is None else np.ascontiguousarray(varFloor, np.float32)
        assert vf is None or vf.shape == (self.D,)
        return UpdateConfig(minEgs, minVar, mixWeightFloor, uFlags, int(singleProcess), None if vf is None else vf.ctypes.data_as(C.POINTER(C.c_float)),
                            int(rowNormalise), mapTau, mapMinObs), vf

    def update(self, accs: "Accs", vec: np.ndarray, minEgs=3, minVar=0.0, mixWeightFloor=0.0, uFlags=UPALL, singleProcess=False, varFloor=None,
               rowNormalise=False, mapTau=20.0, mapMinObs=0.0):
        """UpdateModels (HERest.c:1326) from a host copy of the (summed) accumulator vector.  varFloor: the ~v "varFloor1" vector.
        uFlags with UPMAP: MAPUpdateModels (HMap.c:413) with prior weight mapTau."""
        vec = np.ascontiguousarray(vec, np.float64)
        cfg, vf = self._update_config(minEgs, minVar, mixWeightFloor, uFlags, singleProcess, varFloor, rowNormalise, mapTau, mapMinObs)
        st = UpdateStats()
        check(lib().htkamd_model_update(self.h, accs.h, _p(vec), C.byref(cfg), C.byref(st)), "model_update")
        return {n: getattr(st, n) for n, _ in UpdateStats._fields_}

    def update_device(self, accs: "Accs", minEgs=3, minVar=0.0, mixWeightFloor=0.0, uFlags=UPALL, singleProcess=False, varFloor=None,
                      rowNormalise=False, stream=None):
        """The same update on the device, from the accumulator vector where it lies (htkamd_model_update_device)."""
        cfg, vf = self._update_config(minEgs, minVar, mixWeightFloor, uFlags, singleProcess, varFloor, rowNormalise)
        st = UpdateStats()
        check(lib().htkamd_model_update_device(self.h, accs.h, C.byref(cfg), C.byref(st), _stream(stream)), "model_update_device")
        return {n: getattr(st, n) for n, _ in UpdateStats._fields_}

    def update_device_begin(self, accs: "Accs", minEgs=3, minVar=0.0, mixWeightFloor=0.0, uFlags=UPALL, singleProcess=False, varFloor=None,
                            rowNormalise=False, stream=None):
        """First half of update_device: every launch and the copy of what the host needs, no wait (htkamd_model_update_device_begin)."""
        cfg, vf = self._update_config(minEgs, minVar, mixWeightFloor, uFlags, singleProcess, varFloor, rowNormalise)
        check(lib().htkamd_model_update_device_begin(self.h, accs.h, C.byref(cfg), _stream(stream)), "model_update_device_begin")

    def update_device_end(self):
        """Second half: waits for the update's copy only and returns the counters (htkamd_model_update_device_end)."""
        st = UpdateStats()
        check(lib().htkamd_model_update_device_end(self.h, C.byref(st)), "model_update_device_end")
        return {n: getattr(st, n) for n, _ in UpdateStats._fields_}

    def get_params(self) -> dict:
        k = self._keep
        out = dict(mean=np.empty((self.G, self.D), np.float32), var=np.empty((self.G, self.D), np.float32),
                   gconst=np.empty(self.G, np.float32), compWeight=np.empty(self.C, np.float32),
                   transP=np.empty(len(k["transP"]), np.float32))
        check(lib().htkamd_model_get_params(self.h, _p(out["mean"]), _p(out["var"]), _p(out["gconst"]),
                                            _p(out["compWeight"]), _p(out["transP"])), "model_get_params")
        if self.full:
            out["invCov"] = self.get_inv_cov()
        return out

    def get_inv_cov(self) -> np.ndarray:
        """FULLC model: the inverse covariances [G, D(D+1)/2], lower triangles packed row-major (htkamd_model_get_inv_cov)."""
        out = np.empty((self.G, self.D * (self.D + 1) // 2), np.float32)
        check(lib().htkamd_model_get_inv_cov(self.h, _p(out)), "model_get_inv_cov")
        return out

    def set_inv_cov(self, invCov, gconst=None):
        """FULLC model: new inverse covariances; gconst None = FixFullGConst(mp, -CovDet(inv)) (htkamd_model_set_inv_cov)."""
        ic = np.ascontiguousarray(invCov, np.float32).reshape(-1)
        gc = None if gconst is None else np.ascontiguousarray(gconst, np.float32)
        check(lib().htkamd_model_set_inv_cov(self.h, _p(ic), _p(gc) if gc is not None else None), "model_set_inv_cov")

    def outp_block(self, X: np.ndarray, states: np.ndarray, mode: int = 0) -> np.ndarray:
        """Scores [T, ns] of the listed tied states (HIP kernel K1), returned frame-major for convenience."""
        X = np.ascontiguousarray(X, np.float32); states = np.ascontiguousarray(states, np.int32)
        T, ns = X.shape[0], len(states)
        if T == 0 or ns == 0:
            return np.empty((T, ns), np.float32)
        dX, dS = DevArray(X), DevArray(states)
        dO = DevArray(nbytes=4 * T * ns)
        check(lib().htkamd_outp_block_mode(self.h, dX.ptr, T, dS.ptr, ns, dO.ptr, T, mode, None), "outp_block")
        if mode & SCORE_F16:
            check(lib().htkamd_model_f16_check(self.h, None), "model_f16_check")      # HTKAMD_ERANGE: repeat with SCORE_BF16
        out = dO.to_host(np.float32, (ns, T))
        return np.ascontiguousarray(out.T)


class Accs(_Handle):
    _destroy = "htkamd_accs_destroy"
    def __init__(self, model: Model):
        self.model = model
        self.h = C.c_void_p()
        check(lib().htkamd_accs_create(model.h, C.byref(self.h)), "accs_create")
        self.lay = AccsLayout()
        check(lib().htkamd_accs_get_layout(self.h, C.byref(self.lay)), "accs_get_layout")

    def zero(self, stream=None):
        check(lib().htkamd_accs_zero(self.h, _stream(stream)), "accs_zero")

    def device_vector(self):
        p = C.c_void_p(); n = C.c_size_t()
        check(lib().htkamd_accs_device_vector(self.h, C.byref(p), C.byref(n)), "accs_device_vector")
        return p.value, n.value

    def download(self) -> dict:
        v = np.empty(self.lay.total, np.float64)
        check(lib().htkamd_accs_download(self.h, _p(v), None), "accs_download")
        return self.split(v)

    def upload_add(self, vec: np.ndarray):
        vec = np.ascontiguousarray(vec, np.float64)
        assert vec.size == self.lay.total
        check(lib().htkamd_accs_upload_add(self.h, _p(vec), None), "accs_upload_add")

    def wire_round(self, stream=None):
        """One rank's share of the fp32-on-the-wire exchange (htkamd_accs_allreduce_wire, HTKAMD_WIRE_F32): the statistics rounded to float once."""
        check(lib().htkamd_accs_wire_round(self.h, _stream(stream)), "accs_wire_round")

    def state_ranges(self, state0: int, state1: int, with_rest: bool = False):
        """htkamd_accs_state_ranges: [(offset, length)] of the vector's ranges that belong to tied states [state0, state1) (+ tr / trOcc with with_rest)"""
        off = (C.c_size_t * 7)(); ln = (C.c_size_t * 7)(); n = C.c_int(0)
        check(lib().htkamd_accs_state_ranges(self.h, state0, state1, int(with_rest), off, ln, C.byref(n)), "accs_state_ranges")
        return [(int(off[k]), int(ln[k])) for k in range(n.value)]

    def _ranges(self, fn, ranges, wire, ptr, stream):
        n = len(ranges)
        off = (C.c_size_t * max(n, 1))(*[r[0] for r in ranges]); ln = (C.c_size_t * max(n, 1))(*[r[1] for r in ranges])
        check(fn(self.h, n, off, ln, wire, ptr, _stream(stream)), "accs ranges")

    def pack_ranges(self, ranges, wire: int, dst_ptr: int, stream=None):
        """htkamd_accs_pack_ranges: the ranges one behind the other into device memory at dst_ptr, as floats (wire = 1) or doubles (0)"""
        self._ranges(lib().htkamd_accs_pack_ranges, ranges, wire, dst_ptr, stream)

    def unpack_ranges(self, ranges, wire: int, src_ptr: int, stream=None):
        self._ranges(lib().htkamd_accs_unpack_ranges, ranges, wire, src_ptr, stream)

    def split(self, v: np.ndarray) -> dict:
        m, L = self.model, self.lay
        GD = m.G * m.D
        return dict(vec=v, mu=v[L.mu:L.mu + GD].reshape(m.G, m.D), muOcc=v[L.muOcc:L.muOcc + m.G],
                    va=v[L.va:L.va + GD].reshape(m.G, m.D), vaOcc=v[L.vaOcc:L.vaOcc + m.G],
                    wt=v[L.wt:L.wt + m.C], wtOcc=v[L.wtOcc:L.tr], tr=v[L.tr:L.trOcc], trOcc=v[L.trOcc:L.nEgs],
                    nEgs=v[L.nEgs:L.nEgs + m.H], totalPr=v[L.totalPr], totalT=v[L.totalT], nUttDone=v[L.nUttDone],
                    nUttSkipped=v[L.nUttSkipped], nEval=v[L.nEval])


def fb_config(pruneInit=NOPRUNE, pruneInc=0.0, pruneLim=NOPRUNE, minFrwdP=10.0, uFlags=UPALL, scoreMode=0):
    return FbConfig(pruneInit, pruneInc, pruneLim, minFrwdP, uFlags, scoreMode)


class ForwardBackward(_Handle):
    """htkamd_fb holder: FBFile (HFB.c:1923) over a batch of utterances."""
    _destroy = "htkamd_fb_destroy"

    def __init__(self, model: Model, debug: bool = False, force_general: bool = False, no_state_path: bool = False, stats_list: str = "auto", no_lr_path: bool = False):
        """stats_list: how the mixture statistics reach the accumulators -- "auto": record list + per-Gaussian reduction,
        "tiny": a 128-record list (everything beyond it takes the direct-atomics fallback), "off": direct atomics only."""
        self.model = model
        self.h = C.c_void_p()
        check(lib().htkamd_fb_create(model.h, C.byref(self.h)), "fb_create")
        flags = (1 if debug else 0) | (2 if force_general else 0) | (4 if no_state_path else 0) | {"auto": 0, "tiny": 8, "off": 16}[stats_list] | (32 if no_lr_path else 0)
        if flags:
            check(lib().htkamd_fb_set_debug(self.h, flags), "fb_set_debug")
        self.nUtt = 0
        self._keep = None

    def prepare(self, dX_ptr: int, frameOff: np.ndarray, labOff: np.ndarray, labs: np.ndarray, stream=None):
        frameOff = np.ascontiguousarray(frameOff, np.int32); labOff = np.ascontiguousarray(labOff, np.int32)
        labs = np.ascontiguousarray(labs, np.int32)
        self.nUtt = len(frameOff) - 1
        self._keep = (frameOff, labOff, labs)
        b = BatchDesc(self.nUtt, dX_ptr, _p(frameOff), _p(labOff), _p(labs))
        check(lib().htkamd_fb_prepare(self.h, C.byref(b), _stream(stream)), "fb_prepare")

    def execute(self, cfg: FbConfig, accs: Accs, stream=None):
        check(lib().htkamd_fb_execute(self.h, C.byref(cfg), accs.h, _stream(stream)), "fb_execute")

    def execute_begin(self, cfg: FbConfig, accs: Accs, stream=None) -> bool:
        """htkamd_fb_execute_begin: the pass but for the state-bucketed mixture statistics; True when those wait for execute_mix."""
        d = C.c_int(0)
        check(lib().htkamd_fb_execute_begin(self.h, C.byref(cfg), accs.h, _stream(stream), C.byref(d)), "fb_execute_begin")
        return bool(d.value)

    def execute_mix(self, state0: int, state1: int, stream=None):
        """htkamd_fb_execute_mix: the mixture statistics of tied states [state0, state1)."""
        check(lib().htkamd_fb_execute_mix(self.h, state0, state1, _stream(stream)), "fb_execute_mix")

    def results_begin(self, stream=None):
        """Queue the copy of the results behind the pass on its stream (htkamd_fb_results_begin); results() then only waits for it."""
        check(lib().htkamd_fb_results_begin(self.h, _stream(stream)), "fb_results_begin")

    def results(self, stream=None):
        pr = np.empty(self.nUtt, np.float64); st = np.empty(self.nUtt, np.int32)
        check(lib().htkamd_fb_results(self.h, _p(pr), _p(st), _stream(stream)), "fb_results")
        return pr, st

    def prepared_current(self) -> bool:
        return bool(lib().htkamd_fb_prepared_current(self.h))

    def frame_states(self) -> int:
        return int(lib().htkamd_fb_frame_states(self.h))

    def kernel_times(self):
        t = (C.c_double * 4)()
        check(lib().htkamd_fb_kernel_times(self.h, t), "fb_kernel_times")
        return list(t)

    def set_event_mode(self, mode: int):
        """htkamd_fb_set_event_mode: 0 events between all kernels (default), 1 the scoring dispatch's own only (the other intervals read -1)."""
        check(lib().htkamd_fb_set_event_mode(self.h, mode), "fb_set_event_mode")

    def kernel_times5(self):
        """seconds: scoring, beta, alpha, left-to-right statistics, mixture statistics (htkamd_fb_kernel_times5)"""
        t = (C.c_double * 5)()
        check(lib().htkamd_fb_kernel_times5(self.h, t), "fb_kernel_times5")
        return list(t)

    def mix_counts(self):
        """(pairs, triples) of the last pass's mixture statistics, -1 where uncounted (htkamd_fb_mix_counts)"""
        t = (C.c_longlong * 2)()
        check(lib().htkamd_fb_mix_counts(self.h, t), "fb_mix_counts")
        return int(t[0]), int(t[1])

    def score_work(self):
        """(issued, issued without the per-state frame ranges, needed) in (wavefront, pair) units of the pair kernels (htkamd_fb_score_work)"""
        t = (C.c_longlong * 3)()
        check(lib().htkamd_fb_score_work(self.h, t), "fb_score_work")
        return int(t[0]), int(t[1]), int(t[2])

    def trellis(self, u: int, want_alpha: bool = True):
        T = C.c_int(); Q = C.c_int(); mN = C.c_int()
        check(lib().htkamd_fb_get_trellis(self.h, u, None, None, None, None, None, None, None,
                                          C.byref(T), C.byref(Q), C.byref(mN), None), "fb_get_trellis")
        T, Q, mN = T.value, Q.value, mN.value
        d = dict(beta=np.empty((T, Q, mN)), alpha=np.empty((T, Q, mN)) if want_alpha else None,
                 outp=np.empty((T, Q, mN), np.float32), qLo=np.zeros(T, np.int32), qHi=np.zeros(T, np.int32),
                 aLo=np.zeros(T, np.int32), aHi=np.zeros(T, np.int32))
        check(lib().htkamd_fb_get_trellis(self.h, u, _p(d["beta"]), _p(d["alpha"]), _p(d["outp"]),
                                          _p(d["qLo"]), _p(d["qHi"]), _p(d["aLo"]), _p(d["aHi"]), None, None, None, None),
              "fb_get_trellis")
        return d


class Viterbi(_Handle):
    """htkamd_viterbi holder: HVite -a forced alignment of a batch (HRec token passing on the label chain)."""
    _destroy = "htkamd_viterbi_destroy"

    def __init__(self, model: Model):
        self.model = model
        self.h = C.c_void_p()
        check(lib().htkamd_viterbi_create(model.h, C.byref(self.h)), "viterbi_create")
        self._keep = None

    def align(self, dX_ptr: int, frameOff, labOff, labs, genBeam: float = 1.0e10, stream=None, scoreMode: int = 0):
        frameOff = np.ascontiguousarray(frameOff, np.int32); labOff = np.ascontiguousarray(labOff, np.int32)
        labs = np.ascontiguousarray(labs, np.int32)
        self._keep = (frameOff, labOff, labs)
        nUtt = len(frameOff) - 1
        b = BatchDesc(nUtt, dX_ptr, _p(frameOff), _p(labOff), _p(labs))
        check(lib().htkamd_viterbi_align_mode(self.h, C.byref(b), genBeam, scoreMode, _stream(stream)), "viterbi_align")
        ns = C.c_size_t(); nm = C.c_size_t()
        check(lib().htkamd_viterbi_sizes(self.h, C.byref(ns), C.byref(nm)), "viterbi_sizes")
        r = dict(segStart=np.empty(ns.value, np.int32), segEnd=np.empty(ns.value, np.int32), segScore=np.empty(ns.value, np.float64),
                 modStart=np.empty(nm.value, np.int32), modEnd=np.empty(nm.value, np.int32), modScore=np.empty(nm.value, np.float64),
                 total=np.empty(nUtt, np.float64), status=np.empty(nUtt, np.int32))
        check(lib().htkamd_viterbi_results(self.h, _p(r["segStart"]), _p(r["segEnd"]), _p(r["segScore"]), _p(r["modStart"]),
                                           _p(r["modEnd"]), _p(r["modScore"]), _p(r["total"]), _p(r["status"]), _stream(stream)), "viterbi_results")
        # split per utterance
        m = self.model
        k = m._keep
        out = []
        so = mo = 0
        for u in range(nUtt):
            ql = labs[labOff[u]:labOff[u + 1]]
            nst = [int(k["transN"][k["hmmTrans"][h]]) - 2 for h in ql]
            n = sum(nst)
            out.append(dict(labs=ql, nStates=nst, segStart=r["segStart"][so:so + n], segEnd=r["segEnd"][so:so + n],
                            segScore=r["segScore"][so:so + n], modStart=r["modStart"][mo:mo + len(ql)],
                            modEnd=r["modEnd"][mo:mo + len(ql)], modScore=r["modScore"][mo:mo + len(ql)],
                            total=r["total"][u], status=int(r["status"][u])))
            so += n; mo += len(ql)
        return out


def format_rec(utt: dict, names, frame_dur: int = 100000):
    """Label lines as HVite -a -f -m writes them: start end s<j> score [model modelscore word] (HRec.c:2300-2335)."""
    lines = []
    k = 0
    for q, (h, ns) in enumerate(zip(utt["labs"], utt["nStates"])):
        first = True
        for j in range(ns):
            if utt["segStart"][k] >= 0:
                s = "%d %d s%d %f" % (utt["segStart"][k] * frame_dur, utt["segEnd"][k] * frame_dur, j + 2, np.float32(utt["segScore"][k]))
                if first:
                    s += " %s %f %s" % (names[h], np.float32(utt["modScore"][q]), names[h])
                    first = False
                lines.append(s)
            k += 1
    return lines


class MfccConfig(C.Structure):
    _fields_ = [("sampPeriod", C.c_double), ("winDur", C.c_double), ("frPeriod", C.c_double),
                ("numChans", C.c_int), ("numCeps", C.c_int), ("cepLifter", C.c_int), ("preEmph", C.c_float),
                ("useHam", C.c_int), ("usePower", C.c_int), ("zMeanSource", C.c_int), ("rawEnergy", C.c_int), ("eNormalise", C.c_int),
                ("loFreq", C.c_float), ("hiFreq", C.c_float), ("cepScale", C.c_float), ("silFloor", C.c_float), ("eScale", C.c_float),
                ("hasC0", C.c_int), ("hasE", C.c_int), ("hasD", C.c_int), ("hasA", C.c_int), ("hasZ", C.c_int),
                ("delWin", C.c_int), ("accWin", C.c_int)]


def mfcc_config(kind="MFCC_0_D_A", sampPeriod=625.0, winDur=250000.0, frPeriod=100000.0, numChans=26, numCeps=12, cepLifter=22,
                preEmph=0.97, useHam=True, usePower=False, zMeanSource=False, rawEnergy=True, eNormalise=True,
                loFreq=-1.0, hiFreq=-1.0, cepScale=1.0, silFloor=50.0, eScale=0.1, delWin=2, accWin=2):
    """HParm configuration variables with their defaults (HParm.c:337-367); `kind` is TARGETKIND."""
    q = kind.upper().split("_")
    if q[0] != "MFCC":
        raise HtkAmdError("only MFCC target kinds are on this path")
    return MfccConfig(sampPeriod, winDur, frPeriod, numChans, numCeps, cepLifter, preEmph, int(useHam), int(usePower), int(zMeanSource),
                      int(rawEnergy), int(eNormalise), loFreq, hiFreq, cepScale, silFloor, eScale,
                      int("0" in q[1:]), int("E" in q[1:]), int("D" in q[1:]), int("A" in q[1:]), int("Z" in q[1:]), delWin, accWin)


class _WaveCoder(_Handle):
    """What Mfcc and FrontEnd share: a batch of waveforms on the device and the table its frames go to.  They differ in the symbols."""
    _num_frames = None

    def _upload(self, waves, tables=1):
        """(batch of the int16 waveforms, DevArray for `tables` tables [sum frames, cols], frameOff for the call to fill, sum frames)"""
        w = _Batch(waves, np.int16, who=type(self).__name__)
        total = sum(int(getattr(lib(), self._num_frames)(C.byref(self.cfg), int(n))) for n in np.diff(w.off))
        return w, DevArray(nbytes=4 * max(total, 1) * self.cols * tables), np.zeros(w.n + 1, np.int32), total


class Mfcc(_WaveCoder):
    """htkamd_mfcc holder: waveform -> MFCC feature matrix on the device (HParm/HSigP front end)."""
    _destroy, _num_frames = "htkamd_mfcc_destroy", "htkamd_mfcc_num_frames"

    def __init__(self, cfg: MfccConfig):
        self.cfg = cfg
        self.h = C.c_void_p()
        check(lib().htkamd_mfcc_create(C.byref(cfg), C.byref(self.h)), "mfcc_create")
        self.cols = lib().htkamd_mfcc_num_cols(C.byref(cfg))

    def compute(self, waves, stream=None):
        """waves: list of int16 arrays.  Returns (DevArray features [sumT, cols], frameOff)."""
        w, dO, frameOff, total = self._upload(waves)
        check(lib().htkamd_mfcc_compute(self.h, w.dev.ptr, _p(w.off), w.n, _p(frameOff), dO.ptr, _stream(stream)), "mfcc_compute")
        assert frameOff[-1] == total
        return dO, frameOff

    def compute_host(self, waves):
        dO, frameOff = self.compute(waves)
        return dO.to_host(np.float32, (int(frameOff[-1]), self.cols)), frameOff


class FrontEndConfig(C.Structure):
    _fields_ = [("base", MfccConfig), ("baseKind", C.c_int), ("lpcOrder", C.c_int), ("compressFact", C.c_float)]


FRONTEND_KINDS = {"MFCC": 6, "FBANK": 7, "MELSPEC": 8, "PLP": 11}
_LPC_KINDS = {"LPC": 1, "LPREFC": 2, "LPCEPSTRA": 3}


def frontend_config(kind="PLP_0_D_A", sampPeriod=625.0, winDur=250000.0, frPeriod=100000.0, numChans=26, numCeps=12, cepLifter=22,
                    preEmph=0.97, useHam=True, usePower=False, zMeanSource=False, rawEnergy=True, eNormalise=True,
                    loFreq=-1.0, hiFreq=-1.0, cepScale=1.0, silFloor=50.0, eScale=0.1, delWin=2, accWin=2,
                    lpcOrder=12, compressFact=0.33) -> FrontEndConfig:
    """htkamd_frontend_config from TARGETKIND (e.g. "PLP_0_D_A", "FBANK_E_D_A_Z", "MELSPEC") and the HParm configuration variables.
    The base kind is passed on as its HTK code; whether the device codes it is decided by the library (htkamd_frontend_num_cols)."""
    q = kind.upper().split("_")
    code = FRONTEND_KINDS.get(q[0], _LPC_KINDS.get(q[0]))
    if code is None:
        raise HtkAmdError("unknown base kind %s in %s" % (q[0], kind))
    base = MfccConfig(sampPeriod, winDur, frPeriod, numChans, numCeps, cepLifter, preEmph, int(useHam), int(usePower), int(zMeanSource),
                      int(rawEnergy), int(eNormalise), loFreq, hiFreq, cepScale, silFloor, eScale,
                      int("0" in q[1:]), int("E" in q[1:]), int("D" in q[1:]), int("A" in q[1:]), int("Z" in q[1:]), delWin, accWin)
    return FrontEndConfig(base, code, lpcOrder, compressFact)


def frontend_num_cols(cfg: FrontEndConfig) -> int:
    """Columns of a row of `cfg`'s output; a refused configuration raises HtkAmdError with the library's reason."""
    n = lib().htkamd_frontend_num_cols(C.byref(cfg))
    check(0 if n >= 0 else n, "frontend_num_cols")
    return n


class Warp(C.Structure):
    """htkamd_warp: WARPFREQ, WARPLCUTOFF, WARPUCUTOFF."""
    _fields_ = [("warpFreq", C.c_float), ("warpLCutoff", C.c_float), ("warpUCutoff", C.c_float)]


class FrontEnd(_WaveCoder):
    """htkamd_frontend holder: waveform -> MFCC / FBANK / MELSPEC / PLP feature matrix on the device.
    warps: [(WARPFREQ, WARPLCUTOFF, WARPUCUTOFF), ...] (1..64) makes a front end with one filterbank per warp (VTLN): compute codes
    every utterance with the warp `warp_index` names for it, compute_grid every utterance under every warp."""
    _destroy, _num_frames = "htkamd_frontend_destroy", "htkamd_frontend_num_frames"

    def __init__(self, cfg: FrontEndConfig, warps=None):
        self.cfg = cfg
        self.h = C.c_void_p()
        self.cols = frontend_num_cols(cfg)
        if warps is None:
            check(lib().htkamd_frontend_create(C.byref(cfg), C.byref(self.h)), "frontend_create")
        else:
            arr = (Warp * max(len(warps), 1))(*[Warp(*w) for w in warps])
            check(lib().htkamd_frontend_create_warped(C.byref(cfg), arr, len(warps), C.byref(self.h)), "frontend_create_warped")
        self.num_warps = lib().htkamd_frontend_num_warps(self.h)

    def compute(self, waves, warp_index=None, stream=None):
        """waves: list of int16 arrays; warp_index: the warp of every utterance (None: the first, or only, one for all).
        Returns (DevArray features [sumT, cols], frameOff)."""
        w, dO, frameOff, total = self._upload(waves)
        if warp_index is None:
            check(lib().htkamd_frontend_compute(self.h, w.dev.ptr, _p(w.off), w.n, _p(frameOff), dO.ptr, _stream(stream)), "frontend_compute")
        else:
            idx = np.ascontiguousarray(warp_index, np.int32)
            if idx.shape != (w.n,):
                raise HtkAmdError("warp_index: one entry per utterance expected")
            check(lib().htkamd_frontend_compute_warped(self.h, w.dev.ptr, _p(w.off), w.n, _p(idx), _p(frameOff), dO.ptr, _stream(stream)),
                  "frontend_compute_warped")
        assert frameOff[-1] == total
        return dO, frameOff

    def compute_host(self, waves, warp_index=None):
        dO, frameOff = self.compute(waves, warp_index)
        return dO.to_host(np.float32, (int(frameOff[-1]), self.cols)), frameOff

    def compute_grid(self, waves, stream=None):
        """Every utterance under every warp.  Returns (DevArray [num_warps, sumT, cols], frameOff): table w is what compute gives with
        every utterance on warp w."""
        w, dO, frameOff, total = self._upload(waves, self.num_warps)
        check(lib().htkamd_frontend_compute_grid(self.h, w.dev.ptr, _p(w.off), w.n, _p(frameOff), dO.ptr, _stream(stream)), "frontend_compute_grid")
        assert frameOff[-1] == total
        return dO, frameOff

    def compute_grid_host(self, waves):
        dO, frameOff = self.compute_grid(waves)
        return dO.to_host(np.float32, (self.num_warps, int(frameOff[-1]), self.cols)), frameOff


def _names_array(names):
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    return arr


def accs_layout(pk: dict) -> AccsLayout:
    d, keep = _desc_from_packed(pk)
    lay = AccsLayout()
    check(lib().htkamd_accs_layout_from_desc(C.byref(d), C.byref(lay)), "accs_layout_from_desc")
    return lay


def hmm_scan_order(names) -> np.ndarray:
    order = np.zeros(len(names), np.int32)
    check(lib().htkamd_hmm_scan_order(_names_array(names), len(names), _p(order)), "hmm_scan_order")
    return order


def accs_dump_file(pk: dict, vec: np.ndarray, names, path: str, uFlags: int = UPALL, sharing=None):
    """sharing: (meanShare, varShare) of Mmf.sharing() for a set with ~u / ~v vectors."""
    d, keep = _desc_from_packed(pk)
    vec = np.ascontiguousarray(vec, np.float64)
    ms, vs = (None, None) if sharing is None else (np.ascontiguousarray(sharing[0], np.int32), np.ascontiguousarray(sharing[1], np.int32))
    check(lib().htkamd_accs_dump_file_shared(C.byref(d), _p(vec), _names_array(names), uFlags, _p(ms), _p(vs), path.encode()), "accs_dump_file")


def accs_load_file(pk: dict, vec: np.ndarray, names, path: str, uFlags: int = UPALL, sharing=None):
    d, keep = _desc_from_packed(pk)
    assert vec.dtype == np.float64 and vec.flags.c_contiguous
    ms, vs = (None, None) if sharing is None else (np.ascontiguousarray(sharing[0], np.int32), np.ascontiguousarray(sharing[1], np.int32))
    check(lib().htkamd_accs_load_file_shared(C.byref(d), _p(vec), _names_array(names), uFlags, _p(ms), _p(vs), path.encode()), "accs_load_file")


def stats_write_file(pk: dict, vec: np.ndarray, names, path: str):
    """HERest -s: state occupation statistics file (htkamd_stats_write_file)."""
    d, keep = _desc_from_packed(pk)
    vec = np.ascontiguousarray(vec, np.float64)
    check(lib().htkamd_stats_write_file(C.byref(d), _p(vec), _names_array(names), path.encode()), "stats_write_file")


def parm_read(path: str):
    """HTK parameter file -> (float32 [T, cols], sampPeriod, kind) through the host C reader (handles _C and _K)."""
    data = C.c_void_p(); T = C.c_int(); cols = C.c_int(); per = C.c_int(); kind = C.c_int()
    check(lib().htkamd_parm_read(path.encode(), C.byref(data), C.byref(T), C.byref(cols), C.byref(per), C.byref(kind)), "parm_read")
    n = T.value * cols.value
    arr = np.ctypeslib.as_array((C.c_float * max(n, 1)).from_address(data.value))[:n].copy().reshape(T.value, cols.value)
    lib().htkamd_free(data)
    return arr, per.value, kind.value


WAVE_HTK, WAVE_WAV = 1, 2


def wave_read(path: str, fmt: int = WAVE_WAV):
    """Waveform file -> (int16 samples, sampPeriod in 100 ns units) through the host C reader."""
    data = C.c_void_p(); n = C.c_long(); per = C.c_double()
    check(lib().htkamd_wave_read(path.encode(), fmt, C.byref(data), C.byref(n), C.byref(per)), "wave_read")
    arr = np.ctypeslib.as_array((C.c_short * max(n.value, 1)).from_address(data.value))[:n.value].copy()
    lib().htkamd_free(data)
    return arr, per.value


def parm_write(path: str, X: np.ndarray, sampPeriod: int, kind: int, withCrc: bool = False):
    X = np.ascontiguousarray(X, np.float32)
    check(lib().htkamd_parm_write(path.encode(), _p(X), X.shape[0], X.shape[1], sampPeriod, kind,
                                  int(withCrc)), "parm_write")


def _stat_batch(who, stat_list, cols=None) -> _Batch:
    """The statics of several utterances [T, cols] (cols None: the first one's) for a qualifier step.  No utterances, no table: refused."""
    if len(stat_list) == 0:
        raise HtkAmdError("%s: an empty list of utterances" % who)
    return _Batch(stat_list, np.float32, np.atleast_1d(stat_list[0]).shape[-1] if cols is None else cols, who)


def parm_add_qualifiers(stat_list, hasD=True, hasA=False, delWin=2, accWin=2) -> "DevArray":
    """Statics of several utterances -> device table with deltas/accelerations (AddQualifiers, HParm.c:1618).
    Returns (DevArray [sum T, cols], frameOff)."""
    b = _stat_batch("parm_add_qualifiers", stat_list)
    T, n = b.host.shape
    cols = n * (1 + int(hasD) + int(hasA))
    dOut = DevArray(nbytes=4 * max(T * cols, 1))
    check(lib().htkamd_parm_add_qualifiers(b.dev.ptr, _p(b.off), b.n, n, int(hasD), int(hasA),
                                           delWin, accWin, dOut.ptr, None), "parm_add_qualifiers")
    return dOut, b.off, cols


def compv(dX_ptr, nFrames: int, D: int, minVar: float = 0.0):
    """htkamd_compv: HCompV's global mean and variance of a device table [nFrames x D]."""
    mean = np.zeros(D, np.float32); var = np.zeros(D, np.float32)
    check(lib().htkamd_compv(dX_ptr, nFrames, D, minVar, _p(mean), _p(var), None), "compv")
    return mean, var


def write_vfloors(path: str, var: np.ndarray, scale: float):
    var = np.ascontiguousarray(var, np.float32)
    check(lib().htkamd_mmf_write_vfloors(path.encode(), _p(var), len(var), scale), "mmf_write_vfloors")


class ParmQuals(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nStat", "nZeroMean", "hasD", "hasA", "hasT", "delWin", "accWin", "thirdWin", "nullECol",
                                       "v1Compat", "simpleDiffs")]


def parm_quals_from_kind(kind: str, nStat: int, delWin=2, accWin=2, thirdWin=2, v1Compat=False, simpleDiffs=False) -> ParmQuals:
    """Qualifier step for tables of base kind + _0/_E statics (`nStat` columns) read with TARGETKIND = `kind`, e.g. "MFCC_E_D_A_N"."""
    q = kind.upper().split("_")[1:]
    nE = int("E" in q) + int("0" in q)
    base = nStat - nE
    nZ = (base + int("0" in q and "N" not in q)) if "Z" in q else 0            # HParm.c:1712-1715
    null = base if ("N" in q and nE) else -1                                   # the column after the base coefficients
    return ParmQuals(nStat, nZ, int("D" in q), int("A" in q), int("T" in q), delWin, accWin, thirdWin, null, int(v1Compat), int(simpleDiffs))


def parm_qualify(stat_list, quals: ParmQuals):
    """htkamd_parm_qualify on the statics of several utterances. Returns (DevArray [sum T, cols], frameOff, cols)."""
    b = _stat_batch("parm_qualify", stat_list, quals.nStat)
    cols = lib().htkamd_parm_quals_cols(C.byref(quals))
    dOut = DevArray(nbytes=4 * max(b.host.shape[0] * cols, 1))
    check(lib().htkamd_parm_qualify(b.dev.ptr, _p(b.off), b.n, C.byref(quals), dOut.ptr, None), "parm_qualify")
    return dOut, b.off, cols


def mask_match(mask: str, name: str):
    """htkamd_mask_match (MaskMatch): the characters the mask's % capture from `name`, or None when it does not match."""
    out = C.create_string_buffer(1024)
    rc = lib().htkamd_mask_match(mask.encode(), name.encode(), out, len(out))
    if rc < 0:
        check(rc, "mask_match")
    return out.value.decode() if rc == 1 else None


def parm_kind_parse(kind: str) -> int:
    return lib().htkamd_parm_kind_parse(kind.encode())


def parm_kind_str(kind: int) -> str:
    buf = C.create_string_buffer(64)
    check(lib().htkamd_parm_kind_str(kind, buf, len(buf)), "parm_kind_str")
    return buf.value.decode()


def cepsnorm_read(path: str, max_dim: int = 4096) -> dict:
    """A <CEPSNORM> side file -> {"kind": code, "nFrames": n or None, "mean": float32 [dim] or None, "var": float32 [dim] or None}."""
    kind = C.c_int(); nf = C.c_int(); dm = C.c_int(); dv = C.c_int()
    mean = np.zeros(max_dim, np.float32); var = np.zeros(max_dim, np.float32)
    check(lib().htkamd_cepsnorm_read(path.encode(), C.byref(kind), C.byref(nf), _p(mean), C.byref(dm), _p(var), C.byref(dv), max_dim), "cepsnorm_read")
    return {"kind": kind.value, "nFrames": nf.value if nf.value >= 0 else None,
            "mean": mean[:dm.value].copy() if dm.value else None, "var": var[:dv.value].copy() if dv.value else None}


def cepsnorm_write(path: str, kind: int, flags: str, nFrames: int = 0, mean=None, var=None):
    """htkamd_cepsnorm_write (ExportNMV): flags = HCompV's -q subsets m, v, mv, nv, nmv."""
    mean = None if mean is None else np.ascontiguousarray(mean, np.float32)
    var = None if var is None else np.ascontiguousarray(var, np.float32)
    dim = len(mean) if mean is not None else (len(var) if var is not None else 0)
    check(lib().htkamd_cepsnorm_write(path.encode(), kind, flags.encode(), nFrames, _p(mean), _p(var), dim), "cepsnorm_write")


def varscale_read(path: str, max_dim: int = 4096) -> np.ndarray:
    v = np.zeros(max_dim, np.float32); dim = C.c_int()
    check(lib().htkamd_varscale_read(path.encode(), _p(v), C.byref(dim), max_dim), "varscale_read")
    return v[:dim.value].copy()


def cepsnorm_check_kinds(targetKind: int, meanKind: int = -1, varKind: int = -1):
    check(lib().htkamd_cepsnorm_check_kinds(targetKind, meanKind, varKind), "cepsnorm_check_kinds")


def cepsnorm_scale(varScale, sideVar, sideNames=None) -> np.ndarray:
    """htkamd_cepsnorm_scale: float32 [nSide, dim] = (float)sqrt(varScale / sideVar), the quotient a float as in the reference."""
    vs = np.ascontiguousarray(varScale, np.float32)
    sv = np.ascontiguousarray(np.atleast_2d(sideVar), np.float32)
    out = np.zeros(sv.shape, np.float32)
    names = None if sideNames is None else (C.c_char_p * len(sideNames))(*[n.encode() for n in sideNames])
    check(lib().htkamd_cepsnorm_scale(_p(vs), len(vs), _p(sv), sv.shape[1], sv.shape[0], names, _p(out)), "cepsnorm_scale")
    return out


def side_stats(dX_ptr, frameOff, uttSide, nSide: int, nCols: int, D: int, stream=None):
    """htkamd_side_stats: per side the fp64 sums and sums of squares [nSide, D] of the first D columns, and the frame counts [nSide]."""
    frameOff = np.ascontiguousarray(frameOff, np.int32); uttSide = np.ascontiguousarray(uttSide, np.int32)
    s = np.zeros((nSide, D), np.float64); q = np.zeros((nSide, D), np.float64); n = np.zeros(nSide, np.int64)
    check(lib().htkamd_side_stats(dX_ptr, _p(frameOff), _p(uttSide), len(uttSide), nSide, nCols, D,
                                  _p(s), _p(q), _p(n), _stream(stream)), "side_stats")
    return s, q, n


def side_stats_finish(s, q, n):
    """htkamd_side_stats_finish: (mean, var) float32 [nSide, D] from the sums."""
    s = np.ascontiguousarray(s, np.float64); q = np.ascontiguousarray(q, np.float64); n = np.ascontiguousarray(n, np.int64)
    mean = np.zeros(s.shape, np.float32); var = np.zeros(s.shape, np.float32)
    check(lib().htkamd_side_stats_finish(_p(s), _p(q), _p(n), s.shape[0], s.shape[1], _p(mean), _p(var)), "side_stats_finish")
    return mean, var


def parm_normalise(dX_ptr, frameOff, uttSide, nSide: int, nCols: int, mean=None, scale=None, stream=None):
    """htkamd_parm_normalise, in place on the device table: row - mean[side] (float32 [nSide, dMean]), then row * scale[side]."""
    frameOff = np.ascontiguousarray(frameOff, np.int32); uttSide = np.ascontiguousarray(uttSide, np.int32)
    mean = None if mean is None else np.ascontiguousarray(np.atleast_2d(mean), np.float32)
    scale = None if scale is None else np.ascontiguousarray(np.atleast_2d(scale), np.float32)
    check(lib().htkamd_parm_normalise(dX_ptr, _p(frameOff), _p(uttSide), len(uttSide), nSide, nCols,
                                      _p(mean), 0 if mean is None else mean.shape[1], _p(scale), 0 if scale is None else scale.shape[1],
                                      _stream(stream)), "parm_normalise")


class ParmStream(_Handle):
    """htkamd_parm_stream holder: the qualifier step in HParm's buffer mode (rows in pushes, observations out with qwin rows of delay)."""
    _destroy = "htkamd_parm_stream_close"

    def __init__(self, quals: ParmQuals, max_rows: int):
        self.h = C.c_void_p()
        self.q = quals
        self.max_rows = max_rows
        check(lib().htkamd_parm_stream_open(C.byref(quals), max_rows, C.byref(self.h)), "parm_stream_open")
        self.cols = lib().htkamd_parm_quals_cols(C.byref(quals))
        self.lookahead = lib().htkamd_parm_stream_lookahead(self.h)

    def push(self, rows: np.ndarray, last: bool = False) -> np.ndarray:
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, self.q.nStat)
        dIn = DevArray(rows) if rows.shape[0] else None
        dOut = DevArray(nbytes=4 * max((rows.shape[0] + self.lookahead) * self.cols, 1))
        n = C.c_int(0)
        check(lib().htkamd_parm_stream_push(self.h, dIn.ptr if dIn else None, rows.shape[0], int(last), dOut.ptr, C.byref(n), None), "parm_stream_push")
        return dOut.to_host(np.float32, (max(rows.shape[0] + self.lookahead, 1), self.cols))[:n.value].copy()


class InputXForm:
    """htkamd_inputxform holder: a global linear input transform -- a model set's (Mmf.input_xform, owned by the set) or a file's
    (InputXForm.read: HParm's MATTRANFN names such a file)."""

    def __init__(self, handle, owned: bool, keep=None):
        L = lib()
        self.h, self.owned, self._keep = handle, owned, keep
        self.name = L.htkamd_inputxform_name(handle).decode()
        self.mask = L.htkamd_inputxform_mask(handle).decode()
        self.kind = L.htkamd_inputxform_parm_kind(handle).decode()
        self.prequal = bool(L.htkamd_inputxform_prequal(handle))
        self.rows, self.cols = L.htkamd_inputxform_rows(handle), L.htkamd_inputxform_cols(handle)
        self.vec_size = L.htkamd_inputxform_vec_size(handle)
        self.matrix = np.ctypeslib.as_array(L.htkamd_inputxform_matrix(handle), (self.rows * self.cols,)).reshape(self.rows, self.cols).copy()
        n = C.c_int(0)
        b = L.htkamd_inputxform_bias(handle, C.byref(n))
        self.bias = np.ctypeslib.as_array(b, (n.value,)).copy() if b else None
        self.logdet = float(L.htkamd_inputxform_logdet(handle))

    @classmethod
    def read(cls, path: str) -> "InputXForm":
        h = C.c_void_p()
        check(lib().htkamd_inputxform_read(str(path).encode(), C.byref(h)), "inputxform_read")
        return cls(h, True)

    def write(self, path: str, binary: bool = False):
        check(lib().htkamd_inputxform_write(self.h, str(path).encode(), int(binary)), "inputxform_write")

    def check_against(self, srcKind: str, targetKind: str, nStat: int, setId: str = "", vecSize: int = 0):
        """htkamd_inputxform_check: the reference's checks of a transform against the data and the set it meets."""
        check(lib().htkamd_inputxform_check(self.h, parm_kind_parse(srcKind), parm_kind_parse(targetKind), nStat,
                                            setId.encode(), vecSize), "inputxform_check")

    def apply(self, stat_list, quals: ParmQuals):
        """htkamd_inputxform_apply: the qualifier step of a transformed set on the statics of several utterances, in the reference's
        order.  Returns (DevArray [sum T, cols], frameOff, cols)."""
        b = _stat_batch("InputXForm.apply", stat_list, quals.nStat)
        cols = lib().htkamd_inputxform_apply_cols(self.h, C.byref(quals))
        dOut = DevArray(nbytes=4 * max(b.host.shape[0] * cols, 1))
        check(lib().htkamd_inputxform_apply(self.h, b.dev.ptr, _p(b.off), b.n, C.byref(quals), dOut.ptr, None), "inputxform_apply")
        return dOut, b.off, cols

    def close(self):
        if self.owned and self.h:
            lib().htkamd_inputxform_free(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parm_xform(dIn_ptr, inCols: int, dOut_ptr, outCols: int, nRows: int, dMat_ptr, mrows: int, mcols: int, stream=None):
    """htkamd_parm_xform: out[r][0..mrows) = M . in[r][0..mcols) in the reference's float arithmetic; asynchronous on `stream`."""
    check(lib().htkamd_parm_xform(dIn_ptr, inCols, dOut_ptr, outCols, nRows, dMat_ptr, mrows, mcols,
                                  _stream(stream)), "parm_xform")


TREE_MERGE, TREE_LEAFSTATS = 1, 2


class TreeQuestion(C.Structure):
    _fields_ = [("name", C.c_char_p), ("patterns", C.POINTER(C.c_char_p)), ("nPatterns", C.c_int)]


class TreeSpec(C.Structure):
    _fields_ = [("threshold", C.c_float), ("macRoot", C.c_char_p), ("itemList", C.c_char_p)]


class TreeDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("state", C.c_int), ("nNodes", C.c_int), ("quest", C.POINTER(C.c_int)), ("no", C.POINTER(C.c_int)),
                ("yes", C.POINTER(C.c_int)), ("leafMacro", C.POINTER(C.c_char_p)), ("nLeaves", C.c_int)]


def _tree_questions(questions):
    keep = []
    arr = (TreeQuestion * max(len(questions), 1))()
    for k, (name, pats) in enumerate(questions):
        pa = (C.c_char_p * max(len(pats), 1))(*[str(x).encode() for x in pats])
        keep.append(pa)
        arr[k] = TreeQuestion(str(name).encode(), pa, len(pats))
    return arr, keep


def read_stats(mmf: "Mmf", path: str):
    """An HERest -s statistics file (htkamd_stats_read_file): (occ float32[numStates], count int32[numPhys])."""
    occ = np.zeros(max(mmf.desc.numStates, 1), np.float32); cnt = np.zeros(max(mmf.desc.numPhys, 1), np.int32)
    check(lib().htkamd_stats_read_file(mmf.h, str(path).encode(), _p(occ), _p(cnt)), "stats_read_file")
    return occ[:mmf.desc.numStates], cnt[:mmf.desc.numPhys]


def trees_write(path: str, questions, trees):
    """An ST trees file (htkamd_trees_write): `trees` = [dict(name, state, quest=[..], no=[..], yes=[..], leaves=[macro, ...])]."""
    qs, keepq = _tree_questions(questions)
    keep = []
    td = (TreeDesc * max(len(trees), 1))()
    for k, t in enumerate(trees):
        n = len(t["quest"])
        a = [(C.c_int * max(n, 1))(*t[key]) for key in ("quest", "no", "yes")]
        lm = (C.c_char_p * max(len(t["leaves"]), 1))(*[str(x).encode() for x in t["leaves"]])
        keep.append((a, lm))
        td[k] = TreeDesc(str(t["name"]).encode(), int(t["state"]), n, a[0], a[1], a[2], lm, len(t["leaves"]))
    check(lib().htkamd_trees_write(str(path).encode(), qs, len(questions), td, len(trees)), "trees_write")


def name_question_answers(names, questions, stream=None) -> np.ndarray:
    """Test aid (htkamd_name_question_answers): the answers of model names to QS questions [(name, [pattern, ...])] on the device,
    uint8[nQ, N] -- DoMatch's * and ? over every pattern of a question."""
    qs, keep = _tree_questions(questions)
    N = len(names)
    na = (C.c_char_p * max(N, 1))(*[str(x).encode() for x in names])
    out = np.zeros((max(len(questions), 1), max(N, 1)), np.uint8)
    check(lib().htkamd_name_question_answers(na, N, qs, len(questions), _p(out), _stream(stream)), "name_question_answers")
    return out[:len(questions), :N]


def synth_last_kernel_ms():
    """(matching, walking): the device time of the last add_unseen / tree_descend / name_question_answers call's kernels in ms."""
    ms = (C.c_float * 2)()
    lib().htkamd_synth_last_kernel_ms(ms)
    return float(ms[0]), float(ms[1])


def tree_split_sums(item_stats, node_items, answers, stream=None) -> np.ndarray:
    """Test aid (htkamd_tree_split_sums): the yes / no sums of one node on the device, float32[nQ, 2, 2D+1] (no side first)."""
    st = np.ascontiguousarray(item_stats, np.float32); it = np.ascontiguousarray(node_items, np.int32); an = np.ascontiguousarray(answers, np.uint8)
    nItems, Cc = st.shape
    nQ = an.shape[0]
    if an.shape != (nQ, nItems) or Cc % 2 != 1:
        raise HtkAmdError("tree_split_sums: bad shapes %s %s" % (st.shape, an.shape))
    out = np.zeros((nQ, 2, Cc), np.float32)
    check(lib().htkamd_tree_split_sums(_p(st), nItems, (Cc - 1) // 2, _p(it), it.size, _p(an), nQ, _p(out),
                                       _stream(stream)), "tree_split_sums")
    return out


class RegTree(_Handle):
    """A regression class tree (htkamd_regtree): what Mmf.regtree built, or -- for the writers alone -- a tree from tables:
    RegTree.from_tables(children=[(left, right) | (0, 0), ...] by node number from 1, components={terminal node: [(model, state, mix), ...]}).
    write(identifier, dir) gives HHEd RC's two files, <identifier>.tree and <identifier>.base."""
    _destroy = "htkamd_regtree_destroy"

    def __init__(self, h):
        self.h = h

    @classmethod
    def from_tables(cls, children, components):
        n = len(children)
        left = (C.c_int * max(n, 1))(*[int(c[0]) for c in children]); right = (C.c_int * max(n, 1))(*[int(c[1]) for c in children])
        off, flat = [0], []
        for i in range(1, n + 1):
            flat += list(components.get(i, ()))
            off.append(len(flat))
        co = (C.c_int * (n + 1))(*off)
        cm = (C.c_char_p * max(len(flat), 1))(*[str(x[0]).encode() for x in flat])
        cs = (C.c_int * max(len(flat), 1))(*[int(x[1]) for x in flat]); cx = (C.c_int * max(len(flat), 1))(*[int(x[2]) for x in flat])
        h = C.c_void_p()
        check(lib().htkamd_regtree_from_tables(n, left, right, co, cm, cs, cx, C.byref(h)), "regtree_from_tables")
        return cls(h)

    @property
    def num_nodes(self) -> int:
        return lib().htkamd_regtree_num_nodes(self.h)

    @property
    def num_terminals(self) -> int:
        return lib().htkamd_regtree_num_terminals(self.h)

    def children(self, node: int):
        """(left, right) of node `node` (from 1); (0, 0) for a terminal."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().htkamd_regtree_children(self.h, node, C.byref(a), C.byref(b)), "regtree_children")
        return a.value, b.value

    def terminal_node(self, base_class: int) -> int:
        """The node of base class `base_class` (from 1); 0 when there is none."""
        return lib().htkamd_regtree_terminal_node(self.h, base_class)

    def components(self, node: int):
        """[(physical model, state, mixture), ...] of a terminal node, in the order of the base class file."""
        n = lib().htkamd_regtree_num_components(self.h, node)
        if n < 0:
            raise HtkAmdError("regtree_num_components failed: %s" % lib().htkamd_last_error().decode())
        out = []
        for i in range(n):
            st, mx = C.c_int(0), C.c_int(0)
            name = lib().htkamd_regtree_component(self.h, node, i, C.byref(st), C.byref(mx))
            out.append((name.decode(), st.value, mx.value))
        return out

    def stats(self):
        """(CalcDistance calls of every split in the order the splits were made, device time of the call's kernels in ms)."""
        n = lib().htkamd_regtree_stats(self.h, None, 0, None)
        it = (C.c_int * max(n, 1))(); ms = C.c_float(0.0)
        lib().htkamd_regtree_stats(self.h, it, n, C.byref(ms))
        return list(it[:n]), float(ms.value)

    def write(self, identifier: str, out_dir=None):
        check(lib().htkamd_regtree_write(self.h, str(identifier).encode(), str(out_dir).encode() if out_dir else None), "regtree_write")


def regtree_probe(mean, sum, sqr, occ, has, steps, stream=None):
    """Test aid (htkamd_regtree_probe): the regression class tree's device steps over given members (mean, sum, sqr float32[G, D], occ
    float32[G], has uint8[G]; the list starts as 0 .. G-1).  `steps` run in order on one device state, each ("node", off, n) or
    ("split", off, n, seeds[2, D]).  Returns (results, list): per step float32[2D+2] for a node step, (counts int32[3] = members left,
    right, CalcDistance calls, float32[2, 2D+2] = the two children) for a split; and the member list int32[G] as the last step left it."""
    mean, sum, sqr = (np.ascontiguousarray(a, np.float32) for a in (mean, sum, sqr))
    occ = np.ascontiguousarray(occ, np.float32); has = np.ascontiguousarray(has, np.uint8)
    if mean.ndim != 2 or sum.shape != mean.shape or sqr.shape != mean.shape or occ.shape != mean.shape[:1] or has.shape != mean.shape[:1]:
        raise HtkAmdError("regtree_probe: bad shapes %s %s %s %s %s" % (mean.shape, sum.shape, sqr.shape, occ.shape, has.shape))
    G, D = mean.shape
    nS = len(steps)
    st = np.zeros((max(nS, 1), 3), np.int32); seeds = np.zeros((max(nS, 1), 2, D), np.float32)
    for s, step in enumerate(steps):
        if step[0] not in ("node", "split") or len(step) != (3 if step[0] == "node" else 4):
            raise HtkAmdError("regtree_probe: step %d is %r" % (s, step[:3]))
        st[s] = (step[0] == "split", step[1], step[2])
        if step[0] == "split":
            seeds[s] = np.asarray(step[3], np.float32).reshape(2, D)
    counts = np.zeros((max(nS, 1), 3), np.int32); fig = np.zeros((max(nS, 1), 2, 2 * D + 2), np.float32); lst = np.zeros(max(G, 1), np.int32)
    check(lib().htkamd_regtree_probe(_p(mean), _p(sum), _p(sqr), _p(occ), _p(has), G, D, _p(st), _p(seeds), nS, _p(counts), _p(fig), _p(lst),
                                     _stream(stream)), "regtree_probe")
    return [(counts[s].copy(), fig[s].copy()) if st[s, 0] else fig[s, 0].copy() for s in range(nS)], lst[:G]


class MllrConfig(C.Structure):
    _fields_ = [("splitThresh", C.c_float), ("minOccThresh", C.c_float), ("useBias", C.c_int), ("nBlocks", C.c_int), ("blockSize", C.POINTER(C.c_int))]


MLLR_NOSET = 1


def mllr_config(split_thresh=0.0, min_occ_thresh=0.0, use_bias=True, blocks=None):
    """(htkamd_mllr_config, the array its blockSize points into).  blocks None: one block of the vector size."""
    b = None if blocks is None else (C.c_int * len(blocks))(*[int(x) for x in blocks])
    return MllrConfig(split_thresh, min_occ_thresh, int(bool(use_bias)), 0 if b is None else len(blocks), b), b


def _tree_tables(children):
    n = len(children)
    return n, np.array([c[0] for c in children], np.int32), np.array([c[1] for c in children], np.int32)


class Mllr(_Handle):
    """A set of MLLR mean transforms (htkamd_xformset): Mllr.estimate from a pass's statistics over a regression class tree, Mllr.read from a
    transform file, Mllr.from_tables from matrices.  Transforms and base classes count from 1."""
    _destroy = "htkamd_xformset_destroy"

    def __init__(self, h, status=0):
        self.h, self.status = h, status      # status MLLR_NOSET: the root's occupation did not exceed the threshold, the set has no transform

    @staticmethod
    def check(mmf, tree, **cfg):
        c, keep = mllr_config(**cfg)
        check(lib().htkamd_mllr_check(mmf.h, tree.h if tree is not None else None, C.byref(c)), "mllr_check")

    @classmethod
    def estimate(cls, mmf, model, accs, tree, stream=None, **cfg):
        c, keep = mllr_config(**cfg)
        h = C.c_void_p()
        rc = lib().htkamd_mllr_estimate(mmf.h, model.h if model is not None else None, accs.h if accs is not None else None,
                                        tree.h if tree is not None else None, C.byref(c), C.byref(h), _stream(stream))
        if rc != MLLR_NOSET:
            check(rc, "mllr_estimate")
        return cls(h, rc)

    @classmethod
    def read(cls, path):
        h = C.c_void_p()
        check(lib().htkamd_xformset_read(str(path).encode(), C.byref(h)), "xformset_read")
        return cls(h)

    @classmethod
    def from_tables(cls, A, bias, class_xform, blocks=None, name="mllr", base_name="rtree.base"):
        A = np.ascontiguousarray(A, np.float32)
        nX, D = A.shape[0], A.shape[1]
        b = None if bias is None else np.ascontiguousarray(bias, np.float32).reshape(nX, D)
        bl = np.array([D] if blocks is None else blocks, np.int32); cx = np.ascontiguousarray(class_xform, np.int32)
        h = C.c_void_p()
        check(lib().htkamd_xformset_from_tables(D, len(bl), _p(bl), int(b is not None), nX, _p(A), _p(b), len(cx), _p(cx), name.encode(), base_name.encode(),
                                                C.byref(h)), "xformset_from_tables")
        return cls(h)

    def set_names(self, name=None, base_name=None):
        check(lib().htkamd_xformset_set_names(self.h, name.encode() if name else None, base_name.encode() if base_name else None), "xformset_set_names")

    @property
    def num_xforms(self) -> int:
        return lib().htkamd_xformset_num_xforms(self.h)

    @property
    def vec_size(self) -> int:
        return lib().htkamd_xformset_vec_size(self.h)

    @property
    def blocks(self):
        n = lib().htkamd_xformset_blocks(self.h, None, 0)
        b = (C.c_int * max(n, 1))()
        lib().htkamd_xformset_blocks(self.h, b, n)
        return list(b[:n])

    @property
    def class_xform(self):
        return [lib().htkamd_xformset_class_xform(self.h, c) for c in range(1, lib().htkamd_xformset_num_classes(self.h) + 1)]

    @property
    def xform_nodes(self):
        return [lib().htkamd_xformset_xform_node(self.h, k) for k in range(1, self.num_xforms + 1)]

    def xform(self, k: int):
        """(A float32[D, D], bias float32[D] or None) of transform k."""
        D = self.vec_size
        A, b = np.zeros((D, D), np.float32), np.zeros(D, np.float32)
        check(lib().htkamd_xformset_xform(self.h, k, _p(A), _p(b)), "xformset_xform")
        return A, (b if lib().htkamd_xformset_use_bias(self.h) else None)

    def node_occ(self):
        n = lib().htkamd_xformset_node_occ(self.h, None, 0)
        o = np.zeros(max(n, 1), np.float64)
        lib().htkamd_xformset_node_occ(self.h, _p(o), n)
        return o[:n]

    def kernel_ms(self):
        ms = (C.c_float * 3)()
        lib().htkamd_xformset_kernel_ms(self.h, ms)
        return list(ms)

    def write(self, path):
        check(lib().htkamd_xformset_write(self.h, str(path).encode()), "xformset_write")

    def apply(self, model, gauss_class=None, stream=None):
        gc = None if gauss_class is None else np.ascontiguousarray(gauss_class, np.int32)
        check(lib().htkamd_mllr_apply(model.h, self.h, _p(gc), _stream(stream)), "mllr_apply")

    @staticmethod
    def restore(model, stream=None):
        check(lib().htkamd_mllr_restore(model.h, _stream(stream)), "mllr_restore")

    @staticmethod
    def gauss_classes(mmf, tree):
        cls = np.zeros(max(mmf.desc.numGauss, 1), np.int32)
        check(lib().htkamd_mllr_gauss_classes(mmf.h, tree.h, _p(cls)), "mllr_gauss_classes")
        return cls[:mmf.desc.numGauss]


def mllr_select(children, node_occ, thresh):
    """ParseNode's choice (htkamd_mllr_select): (status, [node of transform 1..], [transform of class 1..])."""
    n, left, right = _tree_tables(children)
    occ = np.ascontiguousarray(node_occ, np.float64)
    nterm = int((left == 0).sum())
    nX = C.c_int(0); xn = np.zeros(n, np.int32); cx = np.zeros(max(nterm, 1), np.int32)
    rc = lib().htkamd_mllr_select(n, _p(left), _p(right), _p(occ), float(thresh), C.byref(nX), _p(xn), _p(cx))
    if rc != MLLR_NOSET:
        check(rc, "mllr_select")
    return rc, xn[:nX.value].tolist(), cx[:nterm].tolist()


def mllr_record_offsets(D, blocks):
    """Row i's place in a node's record of mllr_probe's statistics: (offset, block start, block size); and the record's length."""
    off, rows = 0, []
    c0 = 0
    for bs in blocks:
        for _ in range(bs):
            rows.append((off, c0, bs)); off += (bs + 1) * (bs + 2) // 2 + bs + 1
        c0 += bs
    return rows, off + 1


def mllr_probe(mean, var, occ, sp_sum, cls, children, stream=None, want_stats=True, **cfg):
    """Test aid (htkamd_mllr_probe): the device steps of Mllr.estimate over tables.  Returns a dict: status (0, MLLR_NOSET), stats
    float64[nNodes, record] (mllr_record_offsets), node_occ, x_node, class_xform, A float32[nX, D, D], bias float32[nX, D], W float64[nX, D,
    maxBlock+1], ms [3].  HTKAMD_ERANGE raises HtkAmdError with .rc, .bad_node, .bad_row."""
    mean = np.ascontiguousarray(mean, np.float32); var = np.ascontiguousarray(var, np.float32)
    occ = np.ascontiguousarray(occ, np.float64); sp = np.ascontiguousarray(sp_sum, np.float64); cls = np.ascontiguousarray(cls, np.int32)
    G, D = mean.shape
    if var.shape != (G, D) or occ.shape != (G,) or sp.shape != (G, D) or cls.shape != (G,):
        raise HtkAmdError("mllr_probe: bad shapes")
    c, keep = mllr_config(**cfg)
    blocks = [D] if c.nBlocks == 0 else list(keep)
    n, left, right = _tree_tables(children)
    nterm = int((left == 0).sum())
    rec = lib().htkamd_mllr_record_len(D, len(blocks), (C.c_int * len(blocks))(*blocks))
    stats = np.zeros((n, max(rec, 1)), np.float64) if want_stats else None
    maxd = max(blocks) + 1
    nocc = np.zeros(n, np.float64); nX = C.c_int(0); xn = np.zeros(n, np.int32); cx = np.zeros(max(nterm, 1), np.int32)
    A = np.zeros((n, D, D), np.float32); b = np.zeros((n, D), np.float32); W = np.zeros((n, D, maxd), np.float64)
    bn, br = C.c_int(0), C.c_int(0); ms = (C.c_float * 3)()
    rc = lib().htkamd_mllr_probe(_p(mean), _p(var), _p(occ), _p(sp), _p(cls), G, D, n, _p(left), _p(right), C.byref(c), _p(stats), 0 if stats is None else stats.size,
                                 _p(nocc), C.byref(nX), _p(xn), _p(cx), _p(A), _p(b), _p(W), C.byref(bn), C.byref(br), ms, _stream(stream))
    if rc not in (0, MLLR_NOSET):
        try:
            check(rc, "mllr_probe")
        except HtkAmdError as e:
            e.bad_node, e.bad_row = bn.value, br.value
            raise
    k = nX.value
    return dict(status=rc, stats=stats, node_occ=nocc, x_node=xn[:k].tolist(), class_xform=cx[:nterm].tolist(), A=A[:k], bias=b[:k], W=W[:k], ms=list(ms))


class ClusterSpec(C.Structure):
    _fields_ = [("byCount", C.c_int), ("value", C.c_float), ("macro", C.c_char_p), ("items", C.c_char_p)]


def cluster_merges(idist, num_req: int = 1, threshold: float = 1.0e15, occ=None, outlier: float = 0.0) -> np.ndarray:
    """Test aid (htkamd_cluster_merges): the merge loop of HHEd's Clustering (and RemOutliers when `occ` is given) on a symmetric distance
    matrix; int32[nMerges, 2], the groups (i, j) of every merge, 1-based in the numbering current at that merge."""
    d = np.ascontiguousarray(idist, np.float32)
    N = d.shape[0]
    if d.shape != (N, N):
        raise HtkAmdError("cluster_merges: a square matrix is expected, got %s" % (d.shape,))
    oc = None if occ is None else np.ascontiguousarray(occ, np.float32)
    if oc is not None and oc.shape != (N,):
        raise HtkAmdError("cluster_merges: %s occupations for %d items" % (oc.shape, N))
    out = np.zeros((max(N, 1), 2), np.int32); n = C.c_int(0)
    check(lib().htkamd_cluster_merges(_p(d), N, _p(oc) if oc is not None else None, num_req, threshold, outlier,
                                      _p(out), C.byref(n)), "cluster_merges")
    return out[:n.value].copy()


def state_distances(mmf: "Mmf", items: str, stream=None) -> np.ndarray:
    """Test aid (htkamd_state_distances): HHEd's StateDistance between the states of an item list, float32[n, n] in the list's order."""
    n = C.c_int(0)
    check(lib().htkamd_state_distances(mmf.h, items.encode(), None, 0, C.byref(n), _stream(stream)), "state_distances")
    out = np.zeros((n.value, n.value), np.float32)
    if n.value:
        check(lib().htkamd_state_distances(mmf.h, items.encode(), _p(out), out.size, C.byref(n), _stream(stream)), "state_distances")
    return out


# ---- HInit on the device (htkamd_hinit, htkamd_flat_cluster)
HINIT_OK, HINIT_EFEWSEGS, HINIT_ESHORT, HINIT_ENOMIX, HINIT_ENOPATH, HINIT_EZEROOCC, HINIT_ECLUSTER = 0, 2121, 2122, 2125, 2126, 2127, 7120
MINMIX = 1.0e-5


class HInitConfig(C.Structure):
    _fields_ = [("maxIter", C.c_int), ("epsilon", C.c_float), ("minVar", C.c_float), ("minSeg", C.c_int), ("mixWeightFloor", C.c_float),
                ("uFlags", C.c_int), ("newModel", C.c_int)]


def hinit_config(max_iter=20, epsilon=1.0e-4, min_var=1.0e-2, min_seg=3, mix_weight_floor=0.0, uflags=UPALL, new_model=True) -> HInitConfig:
    """HInit's switches -i -e -v -m -w (as MINMIX * f) -u -n (new_model False = -n: no uniform segmentation)."""
    return HInitConfig(int(max_iter), float(epsilon), float(min_var), int(min_seg), float(mix_weight_floor), int(uflags), int(bool(new_model)))


def _hinit_tokens(tokens):
    t = np.ascontiguousarray(tokens, np.int32).reshape(-1, 3)
    return [np.ascontiguousarray(t[:, k]) for k in range(3)]


def _unit_train(sym, model, n_frames, tokens, cfg, models, run=None, extra=()):
    """htkamd_<sym>_check on a packed description, and with run = (dX_ptr, stream) htkamd_<sym> itself -- HInit and HRest, one core on the C
    side (csrc/unit_train.h) and here.  extra: the names of the int32 [models, maxIter] outputs behind logP.  Returns (model, results)."""
    fr, ln, md = _hinit_tokens(tokens)
    mo = np.ascontiguousarray(models, np.int32)
    n = len(mo)
    task = (int(n_frames), len(fr), _p(fr), _p(ln), _p(md), C.byref(cfg), n, _p(mo))
    if not isinstance(model, Model):
        d, keep = _desc_from_packed(model)
        check(getattr(lib(), "htkamd_%s_check" % sym)(C.byref(d), *task), sym + "_check")
        if run is None:
            return None
        model = Model(model)
    n1, it = max(n, 1), max(cfg.maxIter, 1)
    status, passes, conv = np.zeros(n1, np.int32), np.zeros(n1, np.int32), np.zeros(n1, np.int32)
    logp = np.zeros((n1, it), np.float32)
    more = {name: np.zeros((n1, it), np.int32) for name in extra}
    check(getattr(lib(), "htkamd_" + sym)(model.h, _stream(run[0]), *task, _p(status), _p(passes), _p(conv), _p(logp), *[_p(a) for a in more.values()],
                                          _stream(run[1])), sym)
    return model, [dict(status=int(status[k]), passes=int(passes[k]), converged=bool(conv[k]), logP=[float(x) for x in logp[k, :passes[k]]],
                        **{name: [int(x) for x in a[k, :passes[k]]] for name, a in more.items()}) for k in range(n)]


def hinit_check(pk: dict, n_frames: int, tokens, cfg: HInitConfig, models):
    """Everything htkamd_hinit refuses before it touches a device, on a packed description (htkamd_hinit_check).  tokens: rows of
    (first frame, frames, physical model)."""
    _unit_train("hinit", pk, n_frames, tokens, cfg, models)


def hinit(model, dX_ptr, n_frames: int, tokens, models, cfg: HInitConfig = None, stream=None):
    """Viterbi training of the listed physical models from labelled tokens in one call (htkamd_hinit).  `model`: a Model, or a packed
    description (checked first, then made a Model: the refusals need no device); tokens: rows of (first frame in the table, frames,
    physical model), the reference's order within each model.  Returns (model, results): results[k] for models[k] is a dict of status
    (HINIT_*), passes, converged and logP (the average log probability of every pass).  The estimates are in the model."""
    return _unit_train("hinit", model, n_frames, tokens, cfg or hinit_config(), models, (dX_ptr, stream))


def hinit_uniform_states(n_emit: int, tok_len) -> np.ndarray:
    """UCollectData's rule as the kernels apply it (htkamd_hinit_uniform_states): the 0-based emitting state of every frame of the tokens."""
    ln = np.ascontiguousarray(tok_len, np.int32)
    out = np.zeros(max(int(ln.sum()), 1), np.int32)
    check(lib().htkamd_hinit_uniform_states(int(n_emit), len(ln), _p(ln), _p(out)), "hinit_uniform_states")
    return out[:int(ln.sum())]


def flat_cluster(dX_ptr, n_rows: int, D: int, pools, nc, min_var: float = 0.0, stream=None):
    """FlatCluster (HTrain.c:763) of several pools in one launch (htkamd_flat_cluster).  pools: a list of row-number arrays into the
    device table dX [n_rows, D]; nc: clusters per pool.  Returns a list of dicts per pool: status, size [nc], centre / var [nc, D],
    assign [items] (a failed pool: status HINIT_ECLUSTER and nothing else)."""
    ncs = np.ascontiguousarray(nc, np.int32).reshape(-1)
    if len(ncs) != len(pools):
        raise HtkAmdError("flat_cluster: %d cluster counts for %d pools" % (len(ncs), len(pools)))
    items, off = _pack([np.asarray(p).reshape(-1) for p in pools], np.int32, who="flat_cluster")
    if items.size == 0:      # a host table, so no _Batch: non-null all the same
        items = np.zeros(1, np.int32)
    tot = max(int(np.clip(ncs, 0, None).sum()), 1)
    size = np.zeros(tot, np.int32); ctr = np.zeros((tot, D), np.float32); var = np.zeros((tot, D), np.float32)
    assign = np.zeros(max(int(off[-1]), 1), np.int32); status = np.zeros(max(len(pools), 1), np.int32)
    check(lib().htkamd_flat_cluster(_stream(dX_ptr), int(n_rows), int(D), len(pools), _p(off), _p(items), _p(ncs), min_var,
                                    _p(size), _p(ctr), _p(var), _p(assign), _p(status), _stream(stream)), "flat_cluster")
    out, c0 = [], 0
    for p in range(len(pools)):
        k = int(ncs[p])
        if status[p] != HINIT_OK:
            out.append(dict(status=int(status[p])))
        else:
            out.append(dict(status=0, size=size[c0:c0 + k].copy(), centre=ctr[c0:c0 + k].copy(), var=var[c0:c0 + k].copy(), assign=assign[off[p]:off[p + 1]].copy()))
        c0 += k
    return out


# ---- HRest on the device (htkamd_hrest)
HREST_OK, HREST_EFEWSEGS, HREST_EZEROOCC, HREST_EFLOORSUM, HREST_ENOUSABLE = 0, 2221, 2222, 2223, 2226


class HRestConfig(C.Structure):
    _fields_ = [("maxIter", C.c_int), ("epsilon", C.c_float), ("minVar", C.c_float), ("minSeg", C.c_int), ("mixWeightFloor", C.c_float),
                ("uFlags", C.c_int), ("segReject", C.c_int), ("vDefunct", C.c_float)]


def hrest_config(max_iter=20, epsilon=1.0e-4, min_var=0.0, min_seg=3, mix_weight_floor=0.0, uflags=UPALL, seg_reject=True, v_defunct=0.0) -> HRestConfig:
    """HRest's switches -i -e -v -m -w (as MINMIX * f) -u -t (seg_reject False = -t) and HREST: VDEFUNCT."""
    return HRestConfig(int(max_iter), float(epsilon), float(min_var), int(min_seg), float(mix_weight_floor), int(uflags), int(bool(seg_reject)), float(v_defunct))


def hrest_check(pk: dict, n_frames: int, tokens, cfg: HRestConfig, models):
    """Everything htkamd_hrest refuses before it touches a device, on a packed description (htkamd_hrest_check).  tokens: rows of
    (first frame, frames, physical model)."""
    _unit_train("hrest", pk, n_frames, tokens, cfg, models)


def hrest_token_counts(pk: dict, tokens, cfg: HRestConfig, models):
    """LoadFile's short-token rejection and main's -m test as the call does them (htkamd_hrest_token_counts, no device): returns
    (keep [tokens] bool, kept [models], status [models])."""
    fr, ln, md = _hinit_tokens(tokens)
    mo = np.ascontiguousarray(models, np.int32)
    off = np.ascontiguousarray(pk["hmmStateOff"], np.int32)
    keep = np.zeros(max(len(ln), 1), np.int32); kept = np.zeros(max(len(mo), 1), np.int32); status = np.zeros(max(len(mo), 1), np.int32)
    check(lib().htkamd_hrest_token_counts(_p(off), len(off) - 1, len(ln), _p(ln), _p(md), C.byref(cfg), len(mo), _p(mo),
                                          _p(keep), _p(kept), _p(status)), "hrest_token_counts")
    return keep[:len(ln)].astype(bool), kept[:len(mo)], status[:len(mo)]


def hrest(model, dX_ptr, n_frames: int, tokens, models, cfg: HRestConfig = None, stream=None):
    """Baum-Welch re-estimation of the listed physical models from labelled tokens in one call (htkamd_hrest).  `model`: a Model, or a
    packed description (checked first, then made a Model: the refusals need no device); tokens: rows of (first frame in the table,
    frames, physical model), the reference's order within each model.  Returns (model, results): results[k] for models[k] is a dict of
    status (HREST_*), passes, converged, logP ("Ave LogProb" of every pass) and used ("using N examples").  The estimates are in the model."""
    return _unit_train("hrest", model, n_frames, tokens, cfg or hrest_config(), models, (dX_ptr, stream), extra=("used",))


class Mmf(_Handle):
    """htkamd_mmf holder: LoadHMMSet / SaveHMMSet for text model definitions (htk_amd/host/mmf.c)."""
    _destroy = "htkamd_mmf_destroy"

    def __init__(self, files=(), hmm_list=None, hmm_dir=None, ext=None):
        L = lib()
        self.h = C.c_void_p()
        check(L.htkamd_mmf_create(C.byref(self.h)), "mmf_create")
        for f in files:
            check(L.htkamd_mmf_read(self.h, str(f).encode(), None), "mmf_read")
        check(L.htkamd_mmf_finish(self.h, hmm_list.encode() if hmm_list else None, hmm_dir.encode() if hmm_dir else None,
                                  ext.encode() if ext else None), "mmf_finish")
        self.kind = L.htkamd_mmf_parm_kind(self.h).decode()
        self._refresh_names()
        vf = L.htkamd_mmf_var_floor(self.h)
        self.var_floor = np.ctypeslib.as_array(vf, (self.desc.vecSize,)).copy() if vf else None
        ic = L.htkamd_mmf_inv_cov(self.h)
        D = self.desc.vecSize
        self.inv_cov = np.ctypeslib.as_array(ic, (self.desc.numGauss * (D * (D + 1) // 2),)).reshape(self.desc.numGauss, -1).copy() if ic else None
        self.cov_kind = "FULLC" if self.inv_cov is not None else "DIAGC"
        self.set_id = L.htkamd_mmf_set_id(self.h).decode()
        xf = L.htkamd_mmf_inputxform(self.h)
        self.input_xform = InputXForm(C.c_void_p(xf), False, keep=self) if xf else None      # <INPUTXFORM>: owned by the set

    def _refresh_names(self):
        """The description and the models' names as the holder has them now (at load, and after add_unseen / compact changed the models)."""
        L = lib()
        self.desc = L.htkamd_mmf_desc(self.h).contents
        self.phys_names = [L.htkamd_mmf_phys_name(self.h, h).decode() for h in range(self.desc.numPhys)]
        n = L.htkamd_mmf_num_logical(self.h)
        self.logical_names = [L.htkamd_mmf_logical_name(self.h, i).decode() for i in range(n)]
        self.logical = {self.logical_names[i]: L.htkamd_mmf_logical_phys(self.h, i) for i in range(n)}

    def refuse_input_xform(self, who: str):
        """For a caller that prepares its observations without looking at the set's transform: a set with <INPUTXFORM> would be trained
        or recognised on untransformed rows.  Such a caller says so and stops (InputXForm.apply is the step it lacks)."""
        if self.input_xform is not None:
            raise HtkAmdError("%s: the model set carries an input transform (<INPUTXFORM> %s), which this program does not apply"
                              % (who, self.input_xform.name))

    def packed(self) -> dict:
        """The flat description as the dict of numpy arrays Model() takes."""
        d = self.desc
        def arr(p, n, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (max(n, 1),))[:n].copy()
        S, Cn, G, nT, H, D = d.numStates, d.numComp, d.numGauss, d.numTrans, d.numPhys, d.vecSize
        transOff = arr(d.transOff, nT + 1, C.c_int); hmmStateOff = arr(d.hmmStateOff, H + 1, C.c_int)
        pk = dict(vecSize=D, numStates=S, numComp=Cn, numGauss=G, numTrans=nT, numPhys=H,
                  stateCompOff=arr(d.stateCompOff, S * max(d.numStreams, 1) + 1, C.c_int), compWeight=arr(d.compWeight, Cn, C.c_float),
                  compGauss=arr(d.compGauss, Cn, C.c_int), mean=arr(d.mean, G * D, C.c_float).reshape(G, D),
                  var=arr(d.var, G * D, C.c_float).reshape(G, D) if d.var else None,
                  gconst=arr(d.gconst, G, C.c_float) if d.gconst else None,
                  transN=arr(d.transN, nT, C.c_int), transOff=transOff, transP=arr(d.transP, int(transOff[-1]), C.c_float),
                  hmmTrans=arr(d.hmmTrans, H, C.c_int), hmmStateOff=hmmStateOff, hmmState=arr(d.hmmState, int(hmmStateOff[-1]), C.c_int),
                  numStreams=max(d.numStreams, 1), dimStream=arr(d.dimStream, D, C.c_int) if d.numStreams > 1 else None, hsKind=int(d.hsKind),
                  streamWeight=arr(d.streamWeight, S * d.numStreams, C.c_float) if (d.numStreams > 1 and d.streamWeight) else None)
        if self.inv_cov is not None:      # FULLC: [G, D(D+1)/2] packed lower triangles; var holds placeholders
            pk["invCov"] = self.inv_cov.copy()
            pk["covKind"] = "FULLC"
        return pk

    def sharing(self):
        """(meanShare, varShare): per Gaussian the number of the ~u / ~v macro its mean / variance is, -1 = private; None if nothing is shared."""
        G = self.desc.numGauss
        ms = np.full(max(G, 1), -1, np.int32); vs = np.full(max(G, 1), -1, np.int32)
        n = lib().htkamd_mmf_sharing(self.h, _p(ms), _p(vs))
        return (ms[:G], vs[:G]) if n > 0 else None

    def mixup(self, target: int, states=None):
        """HHEd's MU command on the loaded set: `target` > 0 components per state (or -target more if negative) for the states
        whose indices are in `states` (None = all).  packed() / write() reflect the new set afterwards."""
        sel = None
        if states is not None:
            sel = np.zeros(self.desc.numStates, np.uint8); sel[list(states)] = 1
        check(lib().htkamd_mmf_mixup(self.h, target, _p(sel) if sel is not None else None), "mmf_mixup")

    def item_list(self, text: str):
        """An HHEd item list of state items, "{ pat.state[i] }": [(physical model, state number)] in the order of the reference's list."""
        n = C.c_int(0)
        check(lib().htkamd_mmf_item_list(self.h, text.encode(), None, None, 0, C.byref(n)), "mmf_item_list")
        ph = np.zeros(max(n.value, 1), np.int32); st = np.zeros(max(n.value, 1), np.int32)
        check(lib().htkamd_mmf_item_list(self.h, text.encode(), _p(ph), _p(st), n.value, C.byref(n)), "mmf_item_list")
        return list(zip(ph[:n.value].tolist(), st[:n.value].tolist()))

    def question_answers(self, name: str, patterns) -> np.ndarray:
        """A QS question's answer per physical model (uint8[numPhys])."""
        qs, keep = _tree_questions([(name, patterns)])
        ans = np.zeros(max(self.desc.numPhys, 1), np.uint8)
        check(lib().htkamd_mmf_question_answers(self.h, qs, _p(ans)), "mmf_question_answers")
        return ans[:self.desc.numPhys]

    def tree_cluster(self, occ, questions, specs, outlier: float = -1.0, merge: bool = True, leaf_stats: bool = True, trees_path=None, stream=None):
        """HHEd's RO / QS / TB / ST on the loaded set (htkamd_mmf_tree_cluster): `occ` the state occupations (read_stats), `questions`
        [(name, [pattern, ...])] in QS order, `specs` [(threshold, macro root, item list)] in TB order.  packed() / write() reflect the
        tied set afterwards.  Returns the warning the call left (a dropped question) or None."""
        occ = np.ascontiguousarray(occ, np.float32)
        if occ.shape != (self.desc.numStates,):
            raise HtkAmdError("tree_cluster: %s occupations for %d states" % (occ.shape, self.desc.numStates))
        qs, keepq = _tree_questions(questions)
        keep = [(str(m).encode(), str(i).encode()) for (_, m, i) in specs]
        ts = (TreeSpec * max(len(specs), 1))(*[TreeSpec(float(specs[k][0]), keep[k][0], keep[k][1]) for k in range(len(specs))])
        flags = (TREE_MERGE if merge else 0) | (TREE_LEAFSTATS if leaf_stats else 0)
        check(lib().htkamd_mmf_tree_cluster(self.h, _p(occ), outlier, qs, len(questions), ts, len(specs), flags,
                                            str(trees_path).encode() if trees_path else None, _stream(stream)), "mmf_tree_cluster")
        msg = lib().htkamd_last_error().decode()
        return msg if "warning" in msg else None

    def load_trees(self, path: str):
        """HHEd's LT command (htkamd_mmf_load_trees): the questions and state trees of an ST file join the trees the holder keeps."""
        check(lib().htkamd_mmf_load_trees(self.h, str(path).encode()), "mmf_load_trees")

    def save_trees(self, path: str):
        """HHEd's ST command for the trees the holder keeps -- left by tree_cluster or loaded by load_trees (htkamd_mmf_save_trees)."""
        check(lib().htkamd_mmf_save_trees(self.h, str(path).encode()), "mmf_save_trees")

    def add_unseen(self, list_path: str, stream=None):
        """HHEd's AU command (htkamd_mmf_add_unseen): the set's models become the names of the list file, the unseen ones synthesised from
        the held trees on the device.  Returns (seen, unseen); phys_names / logical / packed() / write() reflect the new set afterwards."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().htkamd_mmf_add_unseen(self.h, str(list_path).encode(), C.byref(a), C.byref(b), _stream(stream)), "mmf_add_unseen")
        self._refresh_names()
        return a.value, b.value

    def compact(self, list_path=None):
        """HHEd's CO command (htkamd_mmf_compact): identical models become one physical model, `list_path` gets the tied list.  Returns
        (logical, physical)."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().htkamd_mmf_compact(self.h, str(list_path).encode() if list_path else None, C.byref(a), C.byref(b)), "mmf_compact")
        self._refresh_names()
        return a.value, b.value

    def trees(self):
        """The held trees: [dict(name, state, nodes, leaves=[~s macro, ...])] in the order of HHEd's tree list."""
        L = lib()
        out = []
        for t in range(L.htkamd_mmf_num_trees(self.h)):
            st, nn, nl = C.c_int(0), C.c_int(0), C.c_int(0)
            name = L.htkamd_mmf_tree_info(self.h, t, C.byref(st), C.byref(nn), C.byref(nl)).decode()
            out.append(dict(name=name, state=st.value, nodes=nn.value, leaves=[L.htkamd_mmf_tree_leaf(self.h, t, k).decode() for k in range(nl.value)]))
        return out

    def tree_descend(self, names, first_state: int, n_states: int, stream=None):
        """Test aid (htkamd_tree_descend): for every name and state number first_state .. first_state+n_states-1 the held tree of the name's
        base phone (-1: none) and the leaf the walk ends in (-1 without a tree): (int32[N, n_states], int32[N, n_states])."""
        N = len(names)
        na = (C.c_char_p * max(N, 1))(*[str(x).encode() for x in names])
        tree = np.zeros((max(N, 1), n_states), np.int32); leaf = np.zeros((max(N, 1), n_states), np.int32)
        check(lib().htkamd_tree_descend(self.h, na, N, first_state, n_states, _p(tree), _p(leaf), _stream(stream)), "tree_descend")
        return tree[:N], leaf[:N]

    def state_macro(self, state: int):
        """The ~s macro name of state `state` of the description, None for an un-named state."""
        r = lib().htkamd_mmf_state_macro(self.h, state)
        return r.decode() if r else None

    def data_cluster(self, occ, specs, outlier: float = -1.0, stream=None):
        """HHEd's TC / NC commands on the loaded set (htkamd_mmf_data_cluster): `occ` the state occupations (read_stats) or None when no
        statistics are loaded (no outlier phase), `specs` [("TC", threshold, macro, item list) | ("NC", count, macro, item list)] in
        script order.  Returns the number of clusters per command; `last_warning` holds the call's warning (an empty list) or None."""
        if occ is not None:
            occ = np.ascontiguousarray(occ, np.float32)
            if occ.shape != (self.desc.numStates,):
                raise HtkAmdError("data_cluster: %s occupations for %d states" % (occ.shape, self.desc.numStates))
        for sp in specs:
            if sp[0] not in ("TC", "NC"):
                raise HtkAmdError("data_cluster: command %s (TC or NC expected)" % (sp[0],))
        keep = [(str(m).encode(), str(i).encode()) for (_, _, m, i) in specs]
        cs = (ClusterSpec * max(len(specs), 1))(*[ClusterSpec(1 if specs[k][0] == "NC" else 0, float(specs[k][1]), keep[k][0], keep[k][1]) for k in range(len(specs))])
        nc = np.zeros(max(len(specs), 1), np.int32)
        check(lib().htkamd_mmf_data_cluster(self.h, _p(occ) if occ is not None else None, outlier, cs, len(specs), _p(nc), _stream(stream)),
              "mmf_data_cluster")
        msg = lib().htkamd_last_error().decode()
        self.last_warning = msg if "warning" in msg else None
        return nc[:len(specs)].tolist()

    def regtree(self, occ, n_terminals: int, item_list=None, stream=None) -> "RegTree":
        """HHEd's RC command on the loaded set (htkamd_mmf_regtree): `occ` the state occupations (read_stats), `item_list` the optional
        list of non-speech states "{ sil.state[2-4].mix }".  The set is not changed; RegTree.write gives the two files."""
        occ = np.ascontiguousarray(occ, np.float32)
        if occ.shape != (self.desc.numStates,):
            raise HtkAmdError("regtree: %s occupations for %d states" % (occ.shape, self.desc.numStates))
        h = C.c_void_p()
        check(lib().htkamd_mmf_regtree(self.h, _p(occ), int(n_terminals), str(item_list).encode() if item_list else None, C.byref(h), _stream(stream)), "mmf_regtree")
        return RegTree(h)

    def tie(self, macro: str, items: str):
        """HHEd's TI command for .state[i] and .transP item lists (htkamd_mmf_tie); host only."""
        check(lib().htkamd_mmf_tie(self.h, str(macro).encode(), str(items).encode()), "mmf_tie")
        msg = lib().htkamd_last_error().decode()
        self.last_warning = msg if "warning" in msg else None

    def write(self, params: dict, one_file=None, out_dir=None, binary=False):
        g = params.get("gconst")
        if self.inv_cov is not None:      # FULLC set: params["invCov"] in place of the variances (htkamd_mmf_write_full)
            if params.get("invCov") is None:
                raise HtkAmdError("mmf_write: a FULLC set is written from params['invCov'] (the packed inverse covariances), which is missing")
            check(lib().htkamd_mmf_write_full(self.h, _p(np.ascontiguousarray(params["mean"], np.float32)), _p(np.ascontiguousarray(params["invCov"], np.float32)),
                                              _p(np.ascontiguousarray(g, np.float32)) if g is not None else None,
                                              _p(np.ascontiguousarray(params["compWeight"], np.float32)), _p(np.ascontiguousarray(params["transP"], np.float32)),
                                              one_file.encode() if one_file else None, out_dir.encode() if out_dir else None, 1 if binary else 0), "mmf_write_full")
            return
        fn = lib().htkamd_mmf_write_binary if binary else lib().htkamd_mmf_write
        check(fn(self.h, _p(np.ascontiguousarray(params["mean"], np.float32)), _p(np.ascontiguousarray(params["var"], np.float32)),
                                     _p(np.ascontiguousarray(g, np.float32)) if g is not None else None,
                                     _p(np.ascontiguousarray(params["compWeight"], np.float32)), _p(np.ascontiguousarray(params["transP"], np.float32)),
                                     one_file.encode() if one_file else None, out_dir.encode() if out_dir else None), "mmf_write")

    def write_sources(self, params: dict, master_out, out_dir=None, binary=False):
        """SaveHMMSet for a set loaded from several master files: master_out[k] = path for the k-th file read (htkamd_mmf_write_sources)."""
        g = params.get("gconst")
        arr = (C.c_char_p * len(master_out))(*[str(x).encode() for x in master_out])
        if self.inv_cov is not None:
            if params.get("invCov") is None:
                raise HtkAmdError("mmf_write_sources: a FULLC set is written from params['invCov'] (the packed inverse covariances), which is missing")
            check(lib().htkamd_mmf_write_sources_full(self.h, _p(np.ascontiguousarray(params["mean"], np.float32)), _p(np.ascontiguousarray(params["invCov"], np.float32)),
                                                      _p(np.ascontiguousarray(g, np.float32)) if g is not None else None,
                                                      _p(np.ascontiguousarray(params["compWeight"], np.float32)), _p(np.ascontiguousarray(params["transP"], np.float32)),
                                                      arr, len(master_out), out_dir.encode() if out_dir else None, 1 if binary else 0), "mmf_write_sources_full")
            return
        check(lib().htkamd_mmf_write_sources(self.h, _p(np.ascontiguousarray(params["mean"], np.float32)), _p(np.ascontiguousarray(params["var"], np.float32)),
                                             _p(np.ascontiguousarray(g, np.float32)) if g is not None else None,
                                             _p(np.ascontiguousarray(params["compWeight"], np.float32)), _p(np.ascontiguousarray(params["transP"], np.float32)),
                                             arr, len(master_out), out_dir.encode() if out_dir else None, 1 if binary else 0), "mmf_write_sources")


def _labels_to_list(h):
    L = lib()
    n = L.htkamd_labels_count(h)
    return [(L.htkamd_labels_name(h, i).decode(), L.htkamd_labels_start(h, i), L.htkamd_labels_end(h, i),
             L.htkamd_labels_score(h, i)) for i in range(n)]


def labels_read(path: str):
    """HTK label file -> [(name, start, end, score)] (htk_amd/host/labio.c)."""
    h = C.c_void_p()
    check(lib().htkamd_labels_read(path.encode(), C.byref(h)), "labels_read")
    out = _labels_to_list(h)
    lib().htkamd_labels_free(h)
    return out


OUT_FLAGS = dict(S=1, W=2, T=4, N=8, X=16, C=32, M=64)       # the letters of HVite -o


class Trans(_Handle):
    """htkamd_trans holder: a transcription being written (labels with up to two auxiliary labels), HVite's -o formatting."""
    _destroy = "htkamd_trans_free"

    def __init__(self, max_aux: int = 0):
        self.h = C.c_void_p()
        check(lib().htkamd_trans_create(max_aux, C.byref(self.h)), "trans_create")

    def add(self, start, end, name, score=0.0, aux1=None, aux1_score=0.0, aux2=None, aux2_score=0.0):
        check(lib().htkamd_trans_add(self.h, start, end, name.encode(), score,
                                     aux1.encode() if aux1 is not None else None, aux1_score,
                                     aux2.encode() if aux2 is not None else None, aux2_score), "trans_add")

    def format(self, frame_dur=100000.0, states=False, models=False, flags=""):
        bits = sum(OUT_FLAGS[c] for c in flags)
        check(lib().htkamd_trans_format(self.h, frame_dur, states, models, bits), "trans_format")

    def write(self, path: str):
        check(lib().htkamd_trans_write(self.h, path.encode()), "trans_write")


class MlfOut:
    def __init__(self, path: str):
        self.h = C.c_void_p()
        check(lib().htkamd_mlf_out_open(path.encode(), C.byref(self.h)), "mlf_out_open")

    def add(self, lab_file: str, trans: Trans):
        check(lib().htkamd_mlf_out_add(self.h, lab_file.encode(), trans.h), "mlf_out_add")

    def close(self):
        if self.h:
            lib().htkamd_mlf_out_close(self.h); self.h = C.c_void_p()


def scp_read(path: str):
    """Script file -> [(logical, physical, start, end)] (start/end -1 = whole file); extended file names are split."""
    L = lib()
    h = C.c_void_p()
    check(L.htkamd_scp_read(path.encode(), C.byref(h)), "scp_read")
    out = [(L.htkamd_scp_logical(h, i).decode(), L.htkamd_scp_physical(h, i).decode(), int(L.htkamd_scp_start(h, i)), int(L.htkamd_scp_end(h, i)))
           for i in range(L.htkamd_scp_count(h))]
    L.htkamd_scp_free(h)
    return out


class Mlf(_Handle):
    _destroy = "htkamd_mlf_free"
    def __init__(self, path: str):
        self.h = C.c_void_p()
        check(lib().htkamd_mlf_read(path.encode(), C.byref(self.h)), "mlf_read")

    def find(self, lab_file: str):
        p = lib().htkamd_mlf_find(self.h, lab_file.encode())
        return None if not p else _labels_to_list(p)

    def entries(self):
        """(pattern, labels handle) of every entry in file order; the handles live as long as this object."""
        L = lib()
        return [(L.htkamd_mlf_pattern(self.h, i).decode(), C.c_void_p(L.htkamd_mlf_entry(self.h, i))) for i in range(L.htkamd_mlf_count(self.h))]


NET_ALLOWXWRDEXP, NET_FORCECXTEXP, NET_FORCELEFTBI, NET_FORCERIGHTBI = 1, 2, 4, 8


class NetDesc(C.Structure):
    _fields_ = [("nNodes", C.c_int), ("nLinks", C.c_int), ("nProns", C.c_int), ("initial", C.c_int), ("final", C.c_int),
                ("kind", C.c_void_p), ("model", C.c_void_p), ("pronProb", C.c_void_p),
                ("linkOff", C.c_void_p), ("linkDest", C.c_void_p), ("linkLike", C.c_void_p)]


class Net(_Handle):
    """htkamd_net holder: SLF word network + dictionary expanded over a model set (htk_amd/host/net.c)."""
    _destroy = "htkamd_net_destroy"

    def __init__(self, slf: str | None, dictionary: str, mmf: "Mmf", words=None, boundary: str | None = None, flags: int = 0):
        """slf: word lattice file; or slf=None and words=[...]: the alignment network of HVite -a for that transcription.
        flags: NET_ALLOWXWRDEXP | NET_FORCECXTEXP | ... (HNet's configuration switches; cross-word context expansion)."""
        L = lib()
        self._mmf = mmf                                    # a cross-word network names models through the set it was built on
        self.h = C.c_void_p()
        if slf is not None:
            check(L.htkamd_net_build_ex(slf.encode(), dictionary.encode(), mmf.h, flags, C.byref(self.h)), "net_build")
        else:
            arr = (C.c_char_p * len(words))(*[w.encode() for w in words])
            check(L.htkamd_net_build_words(arr, len(words), boundary.encode() if boundary else None, dictionary.encode(),
                                           mmf.h, C.byref(self.h)), "net_build_words")
        self._fill()

    def _fill(self):
        """What the holder keeps of a built network."""
        L = lib()
        self.desc = L.htkamd_net_get(self.h).contents
        self.out_syms = [L.htkamd_net_out_sym(self.h, k).decode() for k in range(self.desc.nProns)]
        self.word_names = [L.htkamd_net_word_name(self.h, k).decode() for k in range(self.desc.nProns)]
        self.xwrd = bool(L.htkamd_net_is_xwrd(self.h))
        self.pron_models = []
        buf = (C.c_int * 256)()
        for k in range(self.desc.nProns):
            n = L.htkamd_net_pron_models(self.h, k, buf, 256)
            self.pron_models.append([int(buf[i]) for i in range(min(n, 256))])

    def seq_models(self, prons):
        """Physical models of a recognised pronunciation sequence, word by word (cross-word contexts applied between neighbours)."""
        L = lib()
        buf = (C.c_int * 256)()
        real = [k for k in prons]
        out = []
        for i, k in enumerate(real):
            prev = next((real[j] for j in range(i - 1, -1, -1) if self.pron_models[real[j]]), -1)
            nxt = next((real[j] for j in range(i + 1, len(real)) if self.pron_models[real[j]]), -1)
            n = L.htkamd_net_seq_models(self.h, k, prev, nxt, buf, 256)
            if n < 0:
                raise HtkAmdError("net_seq_models: " + L.htkamd_last_error().decode())
            out.append([int(buf[j]) for j in range(min(n, 256))])
        return out

    def arrays(self) -> dict:
        d = self.desc
        def arr(p, n, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (max(n, 1),))[:n].copy()
        return dict(kind=arr(d.kind, d.nNodes, C.c_int), model=arr(d.model, d.nNodes, C.c_int), pronProb=arr(d.pronProb, d.nNodes, C.c_float),
                    linkOff=arr(d.linkOff, d.nNodes + 1, C.c_int), linkDest=arr(d.linkDest, d.nLinks, C.c_int),
                    linkLike=arr(d.linkLike, d.nLinks, C.c_float), initial=d.initial, final=d.final)


class DecodeConfig(C.Structure):
    _fields_ = [("genBeam", C.c_float), ("wordBeam", C.c_float), ("lmScale", C.c_float), ("wordPen", C.c_float), ("prScale", C.c_float),
                ("scoreMode", C.c_int), ("maxActive", C.c_int)]


# htkamd_decode_out's fields in order, with the type of the array each points to
_DECODE_OUT = dict(nWords=np.int32, wordPron=np.int32, wordStart=np.int32, wordEnd=np.int32, wordScore=np.float32, wordLm=np.float32, wordAc=np.float32,
                   wordLike=np.float64, total=np.float64, finalLm=np.float32)


class DecodeOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _DECODE_OUT]


class LatticeOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("nNodes", "nArcs", "nodeFrame", "nodePron", "nodeNet", "nodeLike", "arcStart", "arcEnd", "arcAc", "arcLm", "arcPr",
                                          "arcScore", "total")]


class LatticeAlignOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("arcAlignOff", "alState", "alModel", "alDur", "alLike")]


class LatticeAlign(C.Structure):
    _fields_ = [("arcAlignOff", C.c_void_p), ("alState", C.c_void_p), ("alModel", C.c_void_p), ("alDur", C.c_void_p), ("alLike", C.c_void_p), ("models", C.c_int)]


class Lattice(C.Structure):
    _fields_ = [("nNodes", C.c_int), ("nArcs", C.c_int), ("nodeFrame", C.c_void_p), ("nodePron", C.c_void_p), ("nodeLike", C.c_void_p),
                ("arcStart", C.c_void_p), ("arcEnd", C.c_void_p), ("arcAc", C.c_void_p), ("arcLm", C.c_void_p), ("arcPr", C.c_void_p),
                ("lmScale", C.c_float), ("wordPen", C.c_float), ("prScale", C.c_float), ("frameDur", C.c_double)]


def _lattice_struct(lat: dict, frame_dur=0.01):
    keep = [np.ascontiguousarray(lat[k], dt) for k, dt in (("nodeFrame", np.int32), ("nodePron", np.int32), ("nodeLike", np.float64), ("arcStart", np.int32),
                                                          ("arcEnd", np.int32), ("arcAc", np.float32), ("arcLm", np.float32), ("arcPr", np.float32))]
    st = Lattice(len(keep[0]), len(keep[3]), *[_p(x) for x in keep], lat["lmScale"], lat["wordPen"], lat["prScale"], frame_dur)
    return st, keep


def lattice_write(lat: dict, net: "Net", path: str, utterance=None, lm_name=None, vocab_name=None, fmt=0, frame_dur=0.01, mmf: "Mmf" = None):
    """htkamd_lattice_write: the SLF file WriteLattice gives for the lattice (fmt: HTKAMD_LAT_* bits, 0 = t v a l; with alignment records in
    `lat` -- Decoder.run_lattice(align=...) -- and the model set `mmf` for the names: 0 = HVite's default t v a l d with durations and likelihoods)."""
    st, keep = _lattice_struct(lat, frame_dur)
    enc = lambda x: x.encode() if x is not None else None
    if "arcAlignOff" in lat and mmf is not None:
        ka = [np.ascontiguousarray(lat[k], dt) for k, dt in (("arcAlignOff", np.int32), ("alState", np.int32), ("alModel", np.int32), ("alDur", np.int32), ("alLike", np.float32))]
        al = LatticeAlign(*[_p(x) for x in ka], 1 if lat.get("alignModels") else 0)
        check(lib().htkamd_lattice_write_align(C.byref(st), C.byref(al), mmf.h, net.h, path.encode(), enc(utterance), enc(lm_name), enc(vocab_name), fmt or 0x3f8), "lattice_write_align")
        return
    check(lib().htkamd_lattice_write(C.byref(st), net.h, path.encode(), enc(utterance), enc(lm_name), enc(vocab_name), fmt or 0x78), "lattice_write")


def lattice_nbest(lat: dict, net: "Net", N: int, frame_dur=0.01, max_len=4096):
    """htkamd_lattice_nbest: up to N alternatives, each a list of (pron, startFrame, endFrame, score) for its arcs."""
    st, keep = _lattice_struct(lat, frame_dur)
    nAlt = C.c_int(0); altLen = np.zeros(N, np.int32); arcs = np.zeros(N * max_len, np.int32)
    check(lib().htkamd_lattice_nbest(C.byref(st), net.h, N, max_len, C.byref(nAlt), _p(altLen), _p(arcs)), "lattice_nbest")
    L = lib()
    out = []
    for i in range(nAlt.value):
        alt = []
        for j in range(int(altLen[i])):
            a_ = int(arcs[i * max_len + j])
            alt.append((int(lat["nodePron"][lat["arcEnd"][a_]]), int(lat["nodeFrame"][lat["arcStart"][a_]]), int(lat["nodeFrame"][lat["arcEnd"][a_]]),
                        float(L.htkamd_lattice_arc_score(C.byref(st), a_))))
        out.append(alt)
    return out


def lattice_nbest_align(lat: dict, net: "Net", mmf: "Mmf", N: int, states=False, models=True, frame_dur=0.01, max_len=4096, flags=""):
    """The N most likely alternatives as the label lines HVite -n N M -m / -f writes: htkamd_lattice_nbest for the arcs,
    htkamd_lattice_align_trans for the labels of the arcs' alignment records, htkamd_trans_format (-o) and the label writer."""
    import tempfile
    st, keep = _lattice_struct(lat, frame_dur)
    ka = [np.ascontiguousarray(lat[k], dt) for k, dt in (("arcAlignOff", np.int32), ("alState", np.int32), ("alModel", np.int32), ("alDur", np.int32), ("alLike", np.float32))]
    al = LatticeAlign(*[_p(x) for x in ka], 1 if lat.get("alignModels") else 0)
    nAlt = C.c_int(0); altLen = np.zeros(N, np.int32); arcs = np.zeros(N * max_len, np.int32)
    check(lib().htkamd_lattice_nbest(C.byref(st), net.h, N, max_len, C.byref(nAlt), _p(altLen), _p(arcs)), "lattice_nbest")
    out = []
    L = lib()
    for i in range(nAlt.value):
        tr = C.c_void_p()
        a_i = np.ascontiguousarray(arcs[i * max_len:i * max_len + int(altLen[i])], np.int32)
        check(L.htkamd_lattice_align_trans(C.byref(st), C.byref(al), mmf.h, net.h, _p(a_i), len(a_i), C.byref(tr)), "lattice_align_trans")
        if not tr.value:
            out.append(None); continue
        check(L.htkamd_trans_format(tr, frame_dur * 1.0e7, int(states), int(models), sum(OUT_FLAGS[c] for c in flags)), "trans_format")
        with tempfile.NamedTemporaryFile("r", suffix=".rec") as f:
            check(L.htkamd_trans_write(tr, f.name.encode()), "trans_write")
            out.append(open(f.name).read().splitlines())
        L.htkamd_trans_free(tr)
    return out


class _LatticeRun(_Batch):
    """The host side of one htkamd_decoder_run_lattice[_align] / htkamd_decoder_set_run_lattice[_align] call: the batch on the device, the
    output arrays and their per-utterance unpacking."""

    def __init__(self, feats, D, maxNodes, maxArcs, align, maxAlign, who):
        _Batch.__init__(self, feats, np.float32, D, who)
        self.maxNodes, self.maxArcs, self.align, self.maxAlign = maxNodes, maxArcs, align, maxAlign
        n1 = max(self.n, 1)
        self.nn = np.zeros(n1, np.int32); self.na = np.zeros(n1, np.int32); self.tot = np.zeros(n1, np.float64)
        self.nF = np.zeros(n1 * maxNodes, np.int32); self.nP = np.zeros_like(self.nF); self.nNet = np.zeros_like(self.nF); self.nL = np.zeros(n1 * maxNodes, np.float64)
        self.aS = np.zeros(n1 * maxArcs, np.int32); self.aE = np.zeros_like(self.aS); self.aAc = np.zeros(n1 * maxArcs, np.float32); self.aLm = np.zeros_like(self.aAc)
        self.aPr = np.zeros_like(self.aAc); self.aSc = np.zeros(n1 * maxArcs, np.float64)
        self.out = LatticeOut(_p(self.nn), _p(self.na), _p(self.nF), _p(self.nP), _p(self.nNet), _p(self.nL), _p(self.aS), _p(self.aE), _p(self.aAc), _p(self.aLm), _p(self.aPr),
                              _p(self.aSc), _p(self.tot))
        if align:
            self.aOff = np.zeros(n1 * (maxArcs + 1), np.int32); self.alS = np.zeros(n1 * maxAlign, np.int32); self.alM = np.zeros_like(self.alS); self.alD = np.zeros_like(self.alS)
            self.alL = np.zeros(n1 * maxAlign, np.float32)
            self.alo = LatticeAlignOut(_p(self.aOff), _p(self.alS), _p(self.alM), _p(self.alD), _p(self.alL))

    def unpack(self, who, lmScale, wordPen, prScale):
        nn, na, maxNodes, maxArcs, maxAlign, align = self.nn, self.na, self.maxNodes, self.maxArcs, self.maxAlign, self.align
        res = []
        for u in range(self.n):
            if nn[u] == -1:
                res.append(None); continue
            if nn[u] < 0:
                raise HtkAmdError("%s: the lattice of utterance %d does not fit (%d)" % (who, u, nn[u]))
            n, a_, o, q = int(nn[u]), int(na[u]), u * maxNodes, u * maxArcs
            res.append(dict(nodeFrame=self.nF[o:o + n].copy(), nodePron=self.nP[o:o + n].copy(), nodeNet=self.nNet[o:o + n].copy(), nodeLike=self.nL[o:o + n].copy(),
                            arcStart=self.aS[q:q + a_].copy(), arcEnd=self.aE[q:q + a_].copy(), arcAc=self.aAc[q:q + a_].copy(), arcLm=self.aLm[q:q + a_].copy(),
                            arcPr=self.aPr[q:q + a_].copy(), arcScore=self.aSc[q:q + a_].copy(), total=float(self.tot[u]), lmScale=lmScale, wordPen=float(wordPen),
                            prScale=float(prScale)))
            if align:
                off = self.aOff[u * (maxArcs + 1):u * (maxArcs + 1) + a_ + 1].copy(); k = int(off[-1]); b = u * maxAlign
                res[-1].update(arcAlignOff=off, alState=self.alS[b:b + k].copy(), alModel=self.alM[b:b + k].copy(), alDur=self.alD[b:b + k].copy(),
                               alLike=self.alL[b:b + k].copy(), alignModels=bool(align & 1))
        return res


class _Decoding(_Handle):
    """What Decoder and DecoderSet share.  They differ in the symbols (_sym_out for the 1-best run, _prefix for the lattice runs) and in
    net_of: None for a Decoder, whose entry points take no netOf argument."""

    def _args(self, method, nU, net_of, genBeam, wordBeam, lmScale, wordPen, prScale, scoreMode, maxActive):
        """(htkamd_decode_config, LM scale, [netOf array] or []) of one run; the refusals name the class and the method the user called."""
        who = "%s.%s" % (type(self).__name__, method)
        lmScale = self.lmScale if lmScale is None else float(lmScale)
        if lmScale != self.lmScale:
            raise HtkAmdError("%s: the LM scale is fixed at creation (LikeToWord look-ahead)" % who)
        if net_of is not None and len(net_of) != nU:
            raise HtkAmdError("%s: %d utterances, %d network indices" % (who, nU, len(net_of)))
        netOf = [] if net_of is None else [np.ascontiguousarray(np.asarray(net_of, np.int64).astype(np.int32) if nU else np.zeros(1, np.int32))]
        return DecodeConfig(genBeam, wordBeam, lmScale, wordPen, prScale, scoreMode, int(maxActive)), lmScale, netOf

    def _run_out(self, feats, net_of, genBeam, wordBeam, lmScale, wordPen, prScale, maxWords, scoreMode, maxActive):
        """htkamd_decoder_run_out / htkamd_decoder_set_run: every array of htkamd_decode_out, [nUtt] / [nUtt, maxWords]."""
        cfg, _, netOf = self._args("run", len(feats), net_of, genBeam, wordBeam, lmScale, wordPen, prScale, scoreMode, maxActive)
        b = _Batch(feats, np.float32, self.model.D, type(self).__name__ + ".run")
        n1 = max(b.n, 1)
        o = {n: np.zeros(n1 if n in ("nWords", "total", "finalLm") else (n1, maxWords), t) for n, t in _DECODE_OUT.items()}
        out = DecodeOut(*[_p(a) for a in o.values()])
        check(getattr(lib(), "htkamd_" + self._sym_out)(self.h, C.byref(cfg), b.dev.ptr, _p(b.off), *map(_p, netOf), b.n, maxWords, C.byref(out), None),
              self._sym_out)
        return {k: v[:b.n] for k, v in o.items()}

    def _words(self, o):
        """Sets last_lm and returns run()'s result from htkamd_decode_out's arrays: per utterance ([(pron, start, end, score), ...] or None, total)."""
        nW = o["nWords"]
        self.last_lm = [[float(o["wordLm"][u, i]) for i in range(max(int(nW[u]), 0))] for u in range(len(nW))]
        return [(None if nW[u] < 0 else [(int(o["wordPron"][u, i]), int(o["wordStart"][u, i]), int(o["wordEnd"][u, i]), float(o["wordScore"][u, i]))
                                         for i in range(nW[u])], float(o["total"][u])) for u in range(len(nW))]

    def _run_lattice(self, feats, net_of, nToks, genBeam, wordBeam, nBeam, lmScale, wordPen, prScale, maxNodes, maxArcs, scoreMode, maxActive, align, maxAlign):
        """htkamd_<_prefix>_run_lattice[_align]: per utterance the lattice as a dict of arrays, or None."""
        cfg, lmScale, netOf = self._args("run_lattice", len(feats), net_of, genBeam, wordBeam, lmScale, wordPen, prScale, scoreMode, maxActive)
        b = _LatticeRun(feats, self.model.D, maxNodes, maxArcs, align, maxAlign, type(self).__name__ + ".run_lattice")
        sym = self._prefix + ("_run_lattice_align" if align else "_run_lattice")      # _align: HVite -n with -m (1) / -f (2), lAlign of every arc
        mode, cap, alo = ([int(align)], [maxAlign], [C.byref(b.alo)]) if align else ([], [], [])      # ... and its three arguments more
        check(getattr(lib(), "htkamd_" + sym)(self.h, C.byref(cfg), nToks, genBeam if nBeam is None else nBeam, *mode, b.dev.ptr, _p(b.off), *map(_p, netOf),
                                              b.n, maxNodes, maxArcs, *cap, C.byref(b.out), *alo, None), sym)
        return b.unpack(self._prefix + "_run_lattice", lmScale, wordPen, prScale)


class Decoder(_Decoding):
    """htkamd_decoder holder: HVite -w (1-best word labels) for a batch of utterances on the device."""
    _destroy, _sym_out, _prefix = "htkamd_decoder_destroy", "decoder_run_out", "decoder"

    def __init__(self, model: "Model", net: "Net", lmScale: float = 1.0):
        self.h = C.c_void_p()
        self.model, self.net, self.lmScale = model, net, float(lmScale)
        check(lib().htkamd_decoder_create(model.h, C.byref(net.desc), lmScale, C.byref(self.h)), "decoder_create")

    def set_order(self, mode: int):
        """htkamd_decoder_set_order: ORDER_AUTO (exact-tie utterances again in HRec's instance order), ORDER_FAST, ORDER_EXACT."""
        check(lib().htkamd_decoder_set_order(self.h, mode), "decoder_set_order")

    def last_tied(self) -> int:
        return int(lib().htkamd_decoder_last_tied(self.h))

    def last_times(self):
        """(scoring ms, token-kernel ms) of the last run, by device events."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        check(lib().htkamd_decoder_last_times(self.h, C.byref(a), C.byref(b)), "decoder_last_times")
        return a.value, b.value

    def last_live(self):
        """(model-instance steps with a live token, without) of the last run's token kernel: htkamd_decoder_last_live."""
        out = (C.c_longlong * 2)()
        check(lib().htkamd_decoder_last_live(self.h, out), "decoder_last_live")
        return int(out[0]), int(out[1])

    def run(self, feats, genBeam=1.0e10, wordBeam=1.0e10, lmScale=None, wordPen=0.0, prScale=1.0, maxWords=1024, scoreMode=0, maxActive=0):
        """feats: list of [T, D] arrays.  Returns per utterance (list of (pron, startFrame, endFrame, score) or None, total)."""
        return self._words(self._run_out(feats, None, genBeam, wordBeam, lmScale, wordPen, prScale, maxWords, scoreMode, maxActive))

    def run_arrays(self, feats, genBeam=1.0e10, wordBeam=1.0e10, lmScale=None, wordPen=0.0, prScale=1.0, maxWords=1024, scoreMode=0, maxActive=0):
        """Every output array of htkamd_decoder_run_out (htkamd_decode_out's fields, [nUtt] / [nUtt, maxWords])."""
        return self._run_out(feats, None, genBeam, wordBeam, lmScale, wordPen, prScale, maxWords, scoreMode, maxActive)

    def run_lattice(self, feats, nToks, genBeam=1.0e10, wordBeam=1.0e10, nBeam=None, lmScale=None, wordPen=0.0, prScale=1.0, maxNodes=20000, maxArcs=80000, scoreMode=0, maxActive=0,
                    align=0, maxAlign=400000):
        """HVite -n nToks [-u maxActive]: per utterance the lattice as a dict of arrays (oracle.decode_nbest's fields + nodePron), or None."""
        return self._run_lattice(feats, None, nToks, genBeam, wordBeam, nBeam, lmScale, wordPen, prScale, maxNodes, maxArcs, scoreMode, maxActive, align, maxAlign)


class DecoderSet(_Decoding):
    """htkamd_decoder_set holder: a batch in which utterance u is decoded against nets[net_of[u]] -- HVite -a from word-level
    transcriptions, HVite -w with a lattice per file (DoAlignment, HVite.c:830) -- in one launch."""
    _destroy, _sym_out, _prefix = "htkamd_decoder_set_destroy", "decoder_set_run", "decoder_set"

    def __init__(self, model: "Model", nets, lmScale: float = 1.0):
        self.h = C.c_void_p()
        self.model, self.nets, self.lmScale = model, list(nets), float(lmScale)
        arr = (C.POINTER(NetDesc) * max(len(self.nets), 1))(*[C.pointer(n.desc) for n in self.nets])
        check(lib().htkamd_decoder_set_create(model.h, arr, len(self.nets), lmScale, C.byref(self.h)), "decoder_set_create")

    def set_order(self, mode: int):
        check(lib().htkamd_decoder_set_set_order(self.h, mode), "decoder_set_set_order")

    def last_tied(self) -> int:
        return int(lib().htkamd_decoder_set_last_tied(self.h))

    def run_arrays(self, feats, net_of, genBeam=1.0e10, wordBeam=1.0e10, lmScale=None, wordPen=0.0, prScale=1.0, maxWords=1024, scoreMode=0, maxActive=0):
        """Every output array of htkamd_decoder_set_run (htkamd_decode_out's fields, [nUtt] / [nUtt, maxWords])."""
        return self._run_out(feats, net_of, genBeam, wordBeam, lmScale, wordPen, prScale, maxWords, scoreMode, maxActive)

    def run(self, feats, net_of, **p):
        """feats: list of [T, D] arrays; net_of[u]: index into the set's networks.  Returns what Decoder.run returns per utterance -- (list of
        (pron, startFrame, endFrame, score) or None, total), pron indexing nets[net_of[u]] -- and sets last_lm and last_status."""
        o = self.run_arrays(feats, net_of, **p)
        self.last_status = [int(x) for x in o["nWords"]]
        return self._words(o)

    def run_lattice(self, feats, net_of, nToks, genBeam=1.0e10, wordBeam=1.0e10, nBeam=None, lmScale=None, wordPen=0.0, prScale=1.0, maxNodes=20000, maxArcs=80000,
                    scoreMode=0, maxActive=0, align=0, maxAlign=400000):
        """HVite -n nToks together with -a or a lattice per file: what Decoder.run_lattice returns per utterance, utterance u over
        nets[net_of[u]] (nodeNet / nodePron index that network) -- htkamd_decoder_set_run_lattice[_align], one launch for the batch."""
        return self._run_lattice(feats, net_of, nToks, genBeam, wordBeam, nBeam, lmScale, wordPen, prScale, maxNodes, maxArcs, scoreMode, maxActive, align, maxAlign)


# ---- scoring recognition output (HResults): htkamd_results_* ----------------------------------------------------------------------

RES_ALIGN, RES_CONF, RES_FULL, RES_TRANS, RES_PSTATS = 1, 2, 4, 8, 16
RES_HIT, RES_SUB, RES_DEL, RES_INS = 0, 1, 2, 3


class ResultsConfig(C.Structure):
    _fields_ = [("nullName", C.c_char_p), ("ignoreCase", C.c_int), ("stripContexts", C.c_int), ("nist", C.c_int), ("nEquiv", C.c_int),
                ("equivClass", C.POINTER(C.c_char_p)), ("equivLabel", C.POINTER(C.c_char_p)), ("nList", C.c_int), ("list", C.POINTER(C.c_char_p)),
                ("refLevel", C.c_int), ("testLevel", C.c_int)]


class ResultsReport(C.Structure):
    _fields_ = [("flags", C.c_int), ("refId", C.c_char_p), ("nRecId", C.c_int), ("recId", C.POINTER(C.c_char_p)), ("nFiles", C.c_int),
                ("recFile", C.POINTER(C.c_char_p)), ("labFile", C.POINTER(C.c_char_p)), ("counts", C.c_void_p), ("alnOff", C.c_void_p), ("aln", C.c_void_p),
                ("totals", C.c_void_p), ("conf", C.c_void_p)]


def _strs(names):
    names = [n.encode() if isinstance(n, str) else n for n in names]
    return (C.c_char_p * max(len(names), 1))(*names)


def results_check_switch(sw: str):
    check(lib().htkamd_results_check_switch(sw.encode()), "results_check_switch")


class Results(_Handle):
    """htkamd_results holder: HResults for K hypothesis sets x U utterances in one call.  equiv: (class, label) pairs in -e order."""
    _destroy = "htkamd_results_destroy"

    def __init__(self, null_name=None, equiv=(), ignore_case=False, strip=False, nist=False, label_list=(), ref_level=0, test_level=0):
        self.h = C.c_void_p()
        self.label_list = list(label_list)
        L = lib()
        cfg = ResultsConfig(None if null_name is None else null_name.encode(), int(ignore_case), int(strip), int(nist), len(equiv), _strs([e[0] for e in equiv]),
                            _strs([e[1] for e in equiv]), len(self.label_list), _strs(self.label_list), int(ref_level), int(test_level))
        check(L.htkamd_results_create(C.byref(cfg), C.byref(self.h)), "results_create")

    def label_id(self, name: str) -> int:
        i = lib().htkamd_results_label_id(self.h, name.encode())
        if i < 0:
            check(i, "results_label_id")
        return i

    def label_name(self, i: int):
        s = lib().htkamd_results_label_name(self.h, i)
        return None if s is None else s.decode()

    def num_labels(self) -> int:
        return int(lib().htkamd_results_num_labels(self.h))

    def add_ref(self, utt: str, names) -> int:
        i = lib().htkamd_results_add_ref(self.h, utt.encode(), len(names), _strs(names))
        if i < 0:
            check(i, "results_add_ref")
        return i

    def ref_for(self, rec_file: str, mlfs=(), lab_dir=None, lab_ext=None):
        """(reference index, its file name as HResults forms it)."""
        buf = C.create_string_buffer(1024)
        arr = (C.c_void_p * max(len(mlfs), 1))(*[m.h for m in mlfs])
        i = lib().htkamd_results_ref_for(self.h, rec_file.encode(), arr, len(mlfs), None if lab_dir is None else lab_dir.encode(),
                                         None if lab_ext is None else lab_ext.encode(), buf, 1024)
        if i < 0:
            check(i, "results_ref_for")
        return i, buf.value.decode()

    def ids(self, labels_handle) -> np.ndarray:
        n = lib().htkamd_labels_count(labels_handle)
        out = np.zeros(max(n, 1), np.int32)
        check(lib().htkamd_results_ids(self.h, labels_handle, _p(out)), "results_ids")
        return out[:n]

    def ids_of(self, names) -> np.ndarray:
        return np.array([self.label_id(n) for n in names], np.int32).reshape(-1)

    def score(self, utt_ref, hyps, align=False, conf=False):
        """hyps[k][u]: id array of set k's hypothesis for utterance u (reference utt_ref[u]).  Returns a dict: counts [K, U, 6] (H D S I N
        status), totals [K, 7] (H D S I N sentences correct), aln: per set, per utterance an [n, 3] array of (op, refId, testId), conf
        [K, V+1, V+1], kernel_ms."""
        K, U = len(hyps), len(utt_ref)
        flat = [np.asarray(h, np.int32).reshape(-1) for hs in hyps for h in hs]
        if len(flat) != K * U:
            raise HtkAmdError("Results.score: every set needs %d hypotheses" % U)
        hypOff = offsets([len(h) for h in flat])      # (the ids stay apart: a closing 0 keeps their host table non-empty)
        hypIds = np.ascontiguousarray(np.concatenate(flat + [np.zeros(1, np.int32)]), np.int32)
        uttRef = np.ascontiguousarray(np.asarray(list(utt_ref) + [0], np.int64).astype(np.int32))
        refLen = [int(lib().htkamd_results_ref_len(self.h, int(u))) for u in utt_ref]
        V = len(self.label_list)
        counts = np.zeros((max(K * U, 1), 6), np.int32)
        totals = np.zeros((max(K, 1), 7), np.int64)
        cap = int(sum(max(r, 0) for r in refLen) * K + hypOff[-1]) if align else 0
        alnOff = np.zeros(K * U + 1, np.int32)
        aln = np.zeros((max(cap, 1), 3), np.int32)
        cm = np.zeros((max(K, 1), V + 1, V + 1), np.int32)
        flags = (RES_ALIGN if align else 0) | (RES_CONF if conf else 0)
        check(lib().htkamd_results_score(self.h, K, U, _p(uttRef), _p(hypOff), _p(hypIds), flags, _p(counts),
                                         _p(alnOff) if align else None, _p(aln) if align else None, cap, _p(totals), _p(cm) if conf else None, None),
              "results_score")
        out = dict(counts=counts[:K * U].reshape(K, U, 6), totals=totals[:K], kernel_ms=float(lib().htkamd_results_last_kernel_ms(self.h)),
                   alnOff=alnOff, alnFlat=aln)
        if align:
            out["aln"] = [[aln[alnOff[k * U + u]:alnOff[k * U + u + 1]] for u in range(U)] for k in range(K)]
        if conf:
            out["conf"] = cm[:K]
        return out

    def write(self, flags, ref_id, rec_ids, rec_files, lab_files, counts, totals, aln_off=None, aln=None, conf=None, path=None, append=False):
        """HResults' text for ONE set: counts [nFiles, 6], totals [7], aln_off [nFiles + 1] into aln [n, 3], conf [V+1, V+1]."""
        n = len(rec_files)
        counts = np.ascontiguousarray(np.asarray(counts, np.int32).reshape(-1, 6) if n else np.zeros((1, 6), np.int32))
        totals = np.ascontiguousarray(totals, np.int64)
        aln_off = None if aln_off is None else np.ascontiguousarray(aln_off, np.int32)
        aln = None if aln is None else np.ascontiguousarray(aln, np.int32)
        conf = None if conf is None else np.ascontiguousarray(conf, np.int32)
        rep = ResultsReport(int(flags), None if ref_id is None else ref_id.encode(), len(rec_ids), _strs(rec_ids), n, _strs(rec_files), _strs(lab_files),
                            _p(counts), _p(aln_off), _p(aln), _p(totals), _p(conf))
        check(lib().htkamd_results_write(self.h, C.byref(rep), None if path is None else path.encode(), int(append)), "results_write")


class LatScales(C.Structure):
    _fields_ = [("acScale", C.c_float), ("lmScale", C.c_float), ("wordPen", C.c_float), ("prScale", C.c_float)]


class LatSetView(C.Structure):
    _fields_ = [("nNodes", C.c_int), ("nArcs", C.c_int), ("start", C.c_int), ("end", C.c_int), ("nodeTime", C.POINTER(C.c_double)), ("nodeWord", C.POINTER(C.c_int)),
                ("nodeVar", C.POINTER(C.c_int)), ("arcStart", C.POINTER(C.c_int)), ("arcEnd", C.POINTER(C.c_int)), ("arcAc", C.POINTER(C.c_float)),
                ("arcLm", C.POINTER(C.c_float)), ("arcPr", C.POINTER(C.c_float)), ("topOrder", C.POINTER(C.c_int)), ("fwdArcs", C.POINTER(C.c_int)),
                ("bwdArcs", C.POINTER(C.c_int))]


class LatBestOut(C.Structure):
    _fields_ = [("nPath", C.c_void_p), ("status", C.c_void_p), ("pathArcs", C.c_void_p), ("totals", C.c_void_p)]


class LatFbOut(C.Structure):
    _fields_ = [("fw", C.c_void_p), ("bw", C.c_void_p), ("best", C.c_void_p)]


LAT_FORMAT = dict(A=0x1, B=0x2, t=0x8, v=0x10, a=0x20, l=0x40, d=0x80, m=0x100, n=0x200, r=0x400)      # the letters of -q


def latset_check_switch(sw: str):
    check(lib().htkamd_latset_check_switch(sw.encode()), "latset_check_switch")


def latset_tile() -> int:
    return int(lib().htkamd_latset_tile())


def lat_scales(settings):
    """settings: rows of (acscale -a, lmscale -s, wdpenalty -p, prscale -r), narrowed to float as HLRescore's assignments narrow them."""
    rows = np.asarray(settings, np.float64).reshape(-1, 4)
    return (LatScales * len(rows))(*[LatScales(*[float(np.float32(x)) for x in r]) for r in rows])


class LatSet(_Handle):
    """htkamd_latset holder: HLRescore for U lattices under K settings in one call.  Per-node results of K settings come back per lattice
    as [nNodes, K] arrays (the library's interleaved layout)."""
    _destroy = "htkamd_latset_destroy"

    def __init__(self, dictionary: str = None, start_word=None, end_word=None, like: "LatSet" = None):
        self.h = C.c_void_p()
        L = lib()
        if like is not None:
            check(L.htkamd_latset_create_like(like.h, C.byref(self.h)), "latset_create_like")
        else:
            check(L.htkamd_latset_create(dictionary.encode(), None if start_word is None else start_word.encode(), None if end_word is None else end_word.encode(),
                                         C.byref(self.h)), "latset_create")

    def __len__(self):
        return int(lib().htkamd_latset_count(self.h))

    def add_file(self, path: str) -> int:
        i = lib().htkamd_latset_add_file(self.h, path.encode())
        if i < 0:
            check(i, "latset_add_file")
        return i

    def add(self, lat: dict, net: "Net", frame_dur=0.01) -> int:
        """A lattice of Decoder.run_lattice / DecoderSet.run_lattice."""
        st, keep = _lattice_struct(lat, frame_dur)
        i = lib().htkamd_latset_add(self.h, C.byref(st), net.h)
        if i < 0:
            check(i, "latset_add")
        return i

    def add_pruned(self, src: "LatSet", u: int, keep_node, keep_arc) -> int:
        kn, ka = np.ascontiguousarray(keep_node, np.uint8), np.ascontiguousarray(keep_arc, np.uint8)
        v = src.view(u)
        if len(kn) != v["nNodes"] or len(ka) != v["nArcs"]:
            raise HtkAmdError("LatSet.add_pruned: the flags do not fit lattice %d" % u)
        i = lib().htkamd_latset_add_pruned(self.h, src.h, u, _p(kn), _p(ka))
        if i < 0:
            check(i, "latset_add_pruned")
        return i

    def view(self, u: int) -> dict:
        v = LatSetView()
        check(lib().htkamd_latset_get(self.h, u, C.byref(v)), "latset_get")
        nn, na = v.nNodes, v.nArcs
        out = dict(nNodes=nn, nArcs=na, start=v.start, end=v.end)
        for f, n in (("nodeTime", nn), ("nodeWord", nn), ("nodeVar", nn), ("topOrder", nn), ("arcStart", na), ("arcEnd", na), ("arcAc", na), ("arcLm", na), ("arcPr", na),
                     ("fwdArcs", na), ("bwdArcs", na)):
            out[f] = np.ctypeslib.as_array(getattr(v, f), shape=(max(n, 1),))[:n].copy()
        out["nullEnd"] = out["nodeWord"][out["arcEnd"]] == 0
        return out

    def word_name(self, w: int):
        s = lib().htkamd_latset_word_name(self.h, int(w))
        return None if s is None else s.decode()

    def sizes(self):
        """(nodes, arcs) per lattice as two int arrays."""
        v = LatSetView()
        nn, na = [], []
        for u in range(len(self)):
            check(lib().htkamd_latset_get(self.h, u, C.byref(v)), "latset_get")
            nn.append(v.nNodes); na.append(v.nArcs)
        return np.array(nn, np.int64), np.array(na, np.int64)

    def _offsets(self):
        nn, na = self.sizes()
        return nn, na, np.concatenate([[0], np.cumsum(nn)]), np.concatenate([[0], np.cumsum(na)])

    def kernel_ms(self) -> float:
        return float(lib().htkamd_latset_last_kernel_ms(self.h))

    def best(self, settings, stream=None) -> dict:
        """LatFindBest for every (setting, lattice): paths[k][u] (arc numbers, start to end), totals [K, U, 4] (ac lm pr tot), status [K, U]."""
        sc = lat_scales(settings); K, U = len(sc), len(self)
        nn, _, noff, _ = self._offsets()
        TN = int(noff[-1])
        nPath, status = np.zeros(max(K * U, 1), np.int32), np.zeros(max(K * U, 1), np.int32)
        arcs, totals = np.zeros(max(K * TN, 1), np.int32), np.zeros((max(K * U, 1), 4), np.float64)
        out = LatBestOut(_p(nPath), _p(status), _p(arcs), _p(totals))
        check(lib().htkamd_latset_best(self.h, K, sc, C.byref(out), _stream(stream)), "latset_best")
        paths = [[arcs[k * TN + noff[u]:k * TN + noff[u] + nPath[k * U + u]].copy() for u in range(U)] for k in range(K)]
        return dict(paths=paths, totals=totals[:K * U].reshape(K, U, 4), status=status[:K * U].reshape(K, U), nPath=nPath, pathArcs=arcs, kernel_ms=self.kernel_ms())

    def fb_max(self, settings, stream=None) -> dict:
        """LatForwBackw(LATFB_MAX): fw[u], bw[u] as [nNodes, K] arrays, best [K, U]."""
        sc = lat_scales(settings); K, U = len(sc), len(self)
        nn, _, noff, _ = self._offsets()
        TN = int(noff[-1])
        fw, bw, best = np.zeros(max(K * TN, 1)), np.zeros(max(K * TN, 1)), np.zeros(max(K * U, 1))
        out = LatFbOut(_p(fw), _p(bw), _p(best))
        check(lib().htkamd_latset_fb_max(self.h, K, sc, C.byref(out), _stream(stream)), "latset_fb_max")
        cut = lambda a: [a[K * noff[u]:K * noff[u + 1]].reshape(int(nn[u]), K) for u in range(U)]
        return dict(fw=cut(fw), bw=cut(bw), best=best[:K * U].reshape(K, U), kernel_ms=self.kernel_ms())

    def prune(self, settings, thresh, arcs_per_sec=None, stream=None) -> dict:
        """LatPrune's survivors: keep_node[k][u], keep_arc[k][u] as boolean arrays."""
        sc = lat_scales(settings); K, U = len(sc), len(self)
        _, _, noff, aoff = self._offsets()
        TN, TA = int(noff[-1]), int(aoff[-1])
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(thresh, np.float64), (K,)))
        aps = np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if arcs_per_sec is None else arcs_per_sec, np.float32), (K,)))
        kn, ka = np.zeros(max(K * TN, 1), np.uint8), np.zeros(max(K * TA, 1), np.uint8)
        check(lib().htkamd_latset_prune(self.h, K, sc, _p(th), _p(aps), _p(kn), _p(ka), _stream(stream)), "latset_prune")
        return dict(keep_node=[[kn[k * TN + noff[u]:k * TN + noff[u + 1]].astype(bool) for u in range(U)] for k in range(K)],
                    keep_arc=[[ka[k * TA + aoff[u]:k * TA + aoff[u + 1]].astype(bool) for u in range(U)] for k in range(K)], kernel_ms=self.kernel_ms())

    def trans(self, u: int, setting, arcs) -> "Trans":
        """LatFindBest's label list for a path of lattice u."""
        a = np.ascontiguousarray(arcs, np.int32)
        t = Trans.__new__(Trans)
        t.h = C.c_void_p()
        check(lib().htkamd_latset_trans(self.h, u, lat_scales([setting]), _p(a), len(a), C.byref(t.h)), "latset_trans")
        return t

    def best_ids(self, results: "Results", best: dict):
        """The K x U best paths as hyps[k][u] id arrays for Results.score."""
        U = len(self); K = len(best["paths"])
        cap = int(best["nPath"].sum()) + 1
        off, ids = np.zeros(K * U + 1, np.int32), np.zeros(cap, np.int32)
        n = lib().htkamd_latset_best_ids(self.h, results.h, K, _p(best["nPath"]), _p(best["pathArcs"]), _p(off), _p(ids), cap)
        if n < 0:
            check(n, "latset_best_ids")
        return [[ids[off[k * U + u]:off[k * U + u + 1]].copy() for u in range(U)] for k in range(K)]

    def write(self, u: int, setting, path: str, node_score=None, fmt: str = None):
        ns = None if node_score is None else np.ascontiguousarray(node_score, np.float64)
        bits = 0 if fmt is None else sum(LAT_FORMAT.get(c, 0) for c in fmt)
        check(lib().htkamd_latset_write(self.h, u, lat_scales([setting]), _p(ns), path.encode(), bits), "latset_write")


# Every struct of include/htk_amd.h and its mirror above: abi.declare reads the pointer returns from it, tests/test_capi_abi.py the layouts.
STRUCTS = {"htkamd_model_desc": ModelDesc, "htkamd_accs_layout": AccsLayout, "htkamd_fb_config": FbConfig, "htkamd_update_config": UpdateConfig,
           "htkamd_update_stats": UpdateStats, "htkamd_batch_desc": BatchDesc, "htkamd_mfcc_config": MfccConfig, "htkamd_frontend_config": FrontEndConfig,
           "htkamd_warp": Warp, "htkamd_parm_quals": ParmQuals, "htkamd_tree_question": TreeQuestion, "htkamd_tree_spec": TreeSpec,
           "htkamd_tree_desc": TreeDesc, "htkamd_cluster_spec": ClusterSpec, "htkamd_hinit_config": HInitConfig, "htkamd_hrest_config": HRestConfig,
           "htkamd_net_desc": NetDesc, "htkamd_decode_config": DecodeConfig, "htkamd_lattice_out": LatticeOut, "htkamd_lattice_align_out": LatticeAlignOut,
           "htkamd_lattice_align": LatticeAlign, "htkamd_lattice": Lattice, "htkamd_decode_out": DecodeOut, "htkamd_results_config": ResultsConfig,
           "htkamd_results_report": ResultsReport, "htkamd_lat_scales": LatScales, "htkamd_latset_view": LatSetView, "htkamd_latset_best_out": LatBestOut,
           "htkamd_latset_fb_out": LatFbOut, "htkamd_mllr_config": MllrConfig}


# ---- label statistics and bigram models (HLStats), word networks (HBuild) ----

LS_DURS, LS_LIST, LS_COUNTS = 1, 2, 4
LM_BACKOFF, LM_MATRIX = 0, 1


def _str_array(words):
    return (C.c_char_p * max(len(words), 1))(*[w.encode() for w in words])


def read_word_list(path: str):
    """The first string of every line: HLStats' label list, HBuild's word list."""
    out = []
    for line in open(path, encoding="latin-1"):
        f = line.split()
        if f:
            out.append(f[0])
    return out


def lstats_probe(V, utts, enter, exit_, wave_cap=None, group_cap=None, times=None, stream=None):
    """htkamd_lstats_probe: the device chain over plain id lists -> dict(count, rowOff, succ, cnt[, durSum, durMin, durMax])."""
    L = lib()
    b = _pack(utts, np.int32, who="lstats_probe")
    ids, off = b
    n = len(ids) + len(utts)
    count, rowOff = np.zeros(V, np.int32), np.zeros(V + 1, np.int32)
    succ, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    st = en = None
    dur = [None, None, None]
    if times is not None:
        st = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64)[:, 0] for t in times]) if len(ids) else np.zeros(0, np.int64))
        en = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64)[:, 1] for t in times]) if len(ids) else np.zeros(0, np.int64))
        dur = [np.zeros(V, np.int64) for _ in range(3)]
    check(L.htkamd_lstats_probe(V, len(utts), _p(off), _p(ids), _p(st), _p(en), enter, exit_, wave_cap or L.htkamd_lstats_wave_cap(), group_cap or L.htkamd_lstats_group_cap(),
                                _p(count), _p(dur[0]), _p(dur[1]), _p(dur[2]), _p(rowOff), _p(succ), _p(cnt), n, _stream(stream)), "lstats_probe")
    out = dict(count=count, rowOff=rowOff, succ=succ[:rowOff[V]].copy(), cnt=cnt[:rowOff[V]].copy())
    if times is not None:
        out.update(durSum=dur[0], durMin=dur[1], durMax=dur[2])
    return out


class LabelStats(_Handle):
    """htkamd_lstats holder: HLStats for a batch of label sequences (csrc/lstats.hip, host/lstats.c)."""
    _destroy = "htkamd_lstats_destroy"

    def __init__(self, words, enter: str = "!ENTER", exit: str = "!EXIT"):
        self.h = C.c_void_p()
        check(lib().htkamd_lstats_create(_str_array(words), len(words), enter.encode(), exit.encode(), C.byref(self.h)), "lstats_create")
        self.n = lib().htkamd_lstats_nwords(self.h)
        self.words = [lib().htkamd_lstats_word(self.h, i).decode("latin-1") for i in range(self.n + 1)]

    def id(self, name: str) -> int:
        return lib().htkamd_lstats_id(self.h, name.encode("latin-1"))

    def ids_of(self, labels_handle):
        """(ids, times [n, 2]) of a label list handle (Mlf.entries(), htkamd_labels_read)."""
        L = lib()
        n = L.htkamd_labels_count(labels_handle)
        ids, st, en = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        check(L.htkamd_lstats_ids(self.h, labels_handle, _p(ids), _p(st), _p(en)), "lstats_ids")
        return ids, np.stack([st, en], 1)

    def count(self, utts, times=None, stream=None):
        """utts: per utterance the ids of its labels; times: per utterance [n, 2] start / end in 100 ns units (for -d), or None."""
        ids, off = _pack(utts, np.int32, who="LabelStats.count")
        st = en = None
        if times is not None:
            t = np.concatenate([np.asarray(x, np.int64).reshape(-1, 2) for x in times]) if len(ids) else np.zeros((0, 2), np.int64)
            st, en = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
        check(lib().htkamd_lstats_count(self.h, len(utts), _p(off), _p(ids), _p(st), _p(en), _stream(stream)), "lstats_count")
        return self

    def plant(self, n_utt, count, rowOff, succ, cnt, dur=None):
        a = [np.ascontiguousarray(x, np.int32) for x in (count, rowOff, succ, cnt)]
        d = [np.ascontiguousarray(x, np.int64) for x in dur] if dur is not None else [None] * 3
        check(lib().htkamd_lstats_plant(self.h, n_utt, _p(a[0]), _p(a[1]), _p(a[2]) if len(a[2]) else None, _p(a[3]) if len(a[3]) else None, _p(d[0]), _p(d[1]), _p(d[2])),
              "lstats_plant")
        return self

    def tables(self) -> dict:
        V = self.n + 1
        count, pcount, rowOff = np.zeros(V, np.int32), np.zeros(V, np.int32), np.zeros(V + 1, np.int32)
        dur = [np.zeros(V, np.int64) for _ in range(3)]
        check(lib().htkamd_lstats_get(self.h, _p(count), _p(pcount), _p(dur[0]), _p(dur[1]), _p(dur[2]), _p(rowOff)), "lstats_get")
        succ, cnt = np.zeros(max(rowOff[V], 1), np.int32), np.zeros(max(rowOff[V], 1), np.int32)
        check(lib().htkamd_lstats_bigrams(self.h, _p(succ), _p(cnt)), "lstats_bigrams")
        return dict(count=count, pcount=pcount, rowOff=rowOff, succ=succ[:rowOff[V]], cnt=cnt[:rowOff[V]], durSum=dur[0], durMin=dur[1], durMax=dur[2])

    def bigram_write(self, path, backoff=False, uni_floor=1.0, big_thresh=0, big_floor=0.0, discount=0.5, trace_path=None):
        check(lib().htkamd_lstats_bigram_write(self.h, path.encode(), int(backoff), uni_floor, big_thresh, big_floor, discount, trace_path.encode() if trace_path else None),
              "lstats_bigram_write")

    def stats_write(self, path, flags, count_limit=0, list_path=None, append=False):
        check(lib().htkamd_lstats_stats_write(self.h, path.encode() if path else None, int(append), flags, count_limit, list_path.encode() if list_path else None),
              "lstats_stats_write")

    @property
    def kernel_ms(self):
        return lib().htkamd_lstats_last_kernel_ms(self.h)


class Bigram(_Handle):
    """htkamd_bigram holder: a back-off or matrix bigram file as ReadLModel reads it."""
    _destroy = "htkamd_bigram_destroy"

    def __init__(self, path: str):
        L = lib()
        self.h = C.c_void_p()
        check(L.htkamd_bigram_read(path.encode(), C.byref(self.h)), "bigram_read")
        self.type, self.n = L.htkamd_bigram_type(self.h), L.htkamd_bigram_nwords(self.h)
        self.words = [None] + [L.htkamd_bigram_word(self.h, i).decode("latin-1") for i in range(1, self.n + 1)]

    def tables(self) -> dict:
        L = lib()
        W = self.n + 1
        if self.type == LM_MATRIX:
            mat = np.zeros((W, W), np.float32)
            check(L.htkamd_bigram_get(self.h, None, None, None, None, None, None, _p(mat)), "bigram_get")
            return dict(mat=mat)
        nb = L.htkamd_bigram_nbigrams(self.h)
        uni, bowt, has, rowOff = np.zeros(W, np.float32), np.zeros(W, np.float32), np.zeros(W, np.int32), np.zeros(W + 1, np.int32)
        succ, prob = np.zeros(max(nb, 1), np.int32), np.zeros(max(nb, 1), np.float32)
        check(L.htkamd_bigram_get(self.h, _p(uni), _p(bowt), _p(has), _p(rowOff), _p(succ), _p(prob), None), "bigram_get")
        return dict(unigram=uni, bowt=bowt, hasEntry=has, rowOff=rowOff, succ=succ[:nb], prob=prob[:nb])


class Network(_Handle):
    """htkamd_wordnet holder: one of HBuild's flat word networks, in memory."""
    _destroy = "htkamd_wordnet_destroy"

    def __init__(self, h):
        self.h = h

    @classmethod
    def word_loop(cls, words, bracket=None):
        h = C.c_void_p()
        b0, b1 = (bracket[0].encode(), bracket[1].encode()) if bracket else (None, None)
        check(lib().htkamd_netbuild_loop(_str_array(words), len(words), b0, b1, C.byref(h)), "netbuild_loop")
        return cls(h)

    @classmethod
    def from_bigram(cls, bigram: Bigram, words, enter="!ENTER", exit="!EXIT", unknown="!NULL", zap_unknown=False, stream=None):
        h = C.c_void_p()
        check(lib().htkamd_netbuild_bigram(bigram.h, _str_array(words), len(words), enter.encode(), exit.encode(), unknown.encode(), int(zap_unknown), C.byref(h),
                                           _stream(stream)), "netbuild_bigram")
        return cls(h)

    def write(self, path: str):
        check(lib().htkamd_wordnet_write(self.h, path.encode()), "wordnet_write")

    def arrays(self) -> dict:
        L = lib()
        lat = L.htkamd_wordnet_lattice(self.h).contents
        def arr(p, n, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (max(n, 1),))[:n].copy()
        pron = arr(lat.nodePron, lat.nNodes, C.c_int)
        return dict(nodeWord=[L.htkamd_wordnet_word(self.h, int(w)).decode("latin-1") if w >= 0 else "!NULL" for w in pron],
                    arcStart=arr(lat.arcStart, lat.nArcs, C.c_int), arcEnd=arr(lat.arcEnd, lat.nArcs, C.c_int), arcLm=arr(lat.arcLm, lat.nArcs, C.c_float))

    def expand(self, dictionary: str, mmf: "Mmf", flags: int = 0) -> "Net":
        """The model-level network for the decoders, as Net(slf, ...) gives it for the written file -- without the file."""
        net = Net.__new__(Net)
        net._mmf = mmf
        net.h = C.c_void_p()
        L = lib()
        n = L.htkamd_wordnet_nwords(self.h)
        words = (C.c_char_p * max(n, 1))(*[L.htkamd_wordnet_word(self.h, w) for w in range(n)])
        check(L.htkamd_net_build_lattice(L.htkamd_wordnet_lattice(self.h), words, n, dictionary.encode(), mmf.h, flags, C.byref(net.h)), "net_build_lattice")
        net._fill()
        return net

    @property
    def kernel_ms(self):
        return lib().htkamd_wordnet_last_kernel_ms(self.h)


def netbuild_probe(mode, N, nodeOf, rowKeep, enter_idx, zap_idx=0, back_node=0, rowOff=None, succ=None, val=None, rowVal=None, uni=None, stream=None):
    """htkamd_netbuild_probe: k_nb_arcs over caller tables -> (arcStart, arcEnd, arcLm)."""
    i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32)
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, np.float32)
    rowOff, succ, nodeOf, rowKeep, val, rowVal, uni = i32(rowOff), i32(succ), i32(nodeOf), i32(rowKeep), f32(val), f32(rowVal), f32(uni)
    cap = (len(succ) + 2 * N) if mode == LM_BACKOFF else N * N
    S, E, Lm, n = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32), C.c_int(0)
    check(lib().htkamd_netbuild_probe(mode, N, _p(rowOff), _p(succ) if succ is not None and len(succ) else None, _p(val), _p(rowVal), _p(uni), _p(nodeOf), _p(rowKeep), enter_idx,
                                      zap_idx, back_node, _p(S), _p(E), _p(Lm), cap, C.byref(n), _stream(stream)), "netbuild_probe")
    return S[:n.value], E[:n.value], Lm[:n.value]
