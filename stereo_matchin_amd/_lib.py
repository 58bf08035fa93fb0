"""ctypes binding of the C-ABI in ``include/asw.h`` (``libasw_hip.so``).

The library is the product: hand-written gfx950 HIP kernels.  There is no CPU
fallback — if the shared object is missing or does not load, every entry point
raises :class:`AswLibraryError`.

``torch`` is imported before the library is opened so that the HIP runtime
already mapped by torch (``libamdhip64.so.7``) is the one the kernels link
against; device pointers and ``hipStream_t`` handles from torch are then valid
arguments.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (must precede loading libasw_hip.so, see module doc)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ASW_LIB overrides the library path (kernel experiments: tools/ builds variants
# of the same sources into another file); the default is the in-tree build.
LIB_PATH = os.environ.get("ASW_LIB") or os.path.join(_HERE, "libasw_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "asw.h")

ASW_OK = 0
ASW_E_INVALID = -1
ASW_E_HIP = -2
ASW_E_NOMEM = -3
ASW_E_UNSUPPORTED = -4
ASW_E_COMM = -5
DISP16_INVALID = 0xFFFF
COMM_ID_BYTES = 128
# the asw_outputs / asw_timings layouts mirrored below (ASW_ABI_VERSION of include/asw.h):
# a library of another revision would write past them, so _load() refuses it
ABI_VERSION = 4

DIR_V = 0
DIR_H = 1
DEN_NONE, DEN_WRITE, DEN_READ = 0, 1, 2  # ASW_DEN_* (cached aggregation denominator)
COLOR_RGB = 0
COLOR_LAB = 1
LR_U8 = 0
LR_NATIVE = 1
# asw_params.flags (ASW_FLAG_*): frame-API context options (ABI 4)
FLAG_COMM_LOCAL = 0x20
FLAG_RAW_F32 = 0x40


class AswLibraryError(RuntimeError):
    """The HIP library is missing or failed to load (no fallback exists)."""


class AswError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = f"{where}: {strerror(status)} ({status})"
        if status == ASW_E_HIP:
            msg += f", hipError={_lib_or_raise().asw_last_hip_error()}"
        super().__init__(msg)


class AswParams(ctypes.Structure):
    """Mirror of ``asw_params`` (include/asw.h)."""

    _fields_ = [
        ("width", ctypes.c_int), ("height", ctypes.c_int),
        ("ndisp", ctypes.c_int), ("taps", ctypes.c_int), ("iters", ctypes.c_int),
        ("gamma_c", ctypes.c_float), ("gamma_g", ctypes.c_float),
        ("color_space", ctypes.c_int), ("tad_tau", ctypes.c_float),
        ("lr_check", ctypes.c_int), ("lr_mode", ctypes.c_int),
        ("d_begin", ctypes.c_int), ("d_end", ctypes.c_int),
        ("flags", ctypes.c_int),
    ]

    def copy(self) -> "AswParams":
        p = AswParams()
        ctypes.pointer(p)[0] = self
        return p

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}

    @property
    def d_stop(self) -> int:
        return self.ndisp if self.d_end < 0 else self.d_end


class AswOutputs(ctypes.Structure):
    _fields_ = [
        ("d_ref", ctypes.c_void_p), ("d_tar", ctypes.c_void_p),
        ("conf_ref", ctypes.c_void_p), ("conf_tar", ctypes.c_void_p),
        ("disp_rgba", ctypes.c_void_p), ("lr_rgba", ctypes.c_void_p),
        ("lr_red_rgba", ctypes.c_void_p), ("cost", ctypes.c_void_p),
        ("final_rgba", ctypes.c_void_p), ("post_red_rgba", ctypes.c_void_p),
        ("disp16", ctypes.c_void_p), ("lr16", ctypes.c_void_p),
    ]


class AswSubpixelOutputs(ctypes.Structure):
    """Mirror of ``asw_subpixel_outputs`` (include/asw.h): host float32 [H][W] arrays."""

    _fields_ = [("disp", ctypes.c_void_p), ("disp_lr", ctypes.c_void_p), ("disp_filled", ctypes.c_void_p)]


class AswRefineNativeOutputs(ctypes.Structure):
    """Mirror of ``asw_refine_native_outputs`` (include/asw.h): host uint16 / int32 [H][W] arrays."""

    _fields_ = [("final16", ctypes.c_void_p), ("post16", ctypes.c_void_p), ("d_ref", ctypes.c_void_p),
                ("d_tar", ctypes.c_void_p)]


class AswRefineParams(ctypes.Structure):
    """Mirror of ``asw_refine_params`` (include/asw.h)."""

    _fields_ = [("iters", ctypes.c_int), ("taps", ctypes.c_int), ("gamma_c", ctypes.c_float),
                ("gamma_g", ctypes.c_float), ("alpha", ctypes.c_float)]


class AswCrossParams(ctypes.Structure):
    """Mirror of ``asw_cross_params`` (include/asw.h)."""

    _fields_ = [("arm_max", ctypes.c_int), ("tau", ctypes.c_int)]


class AswCensusParams(ctypes.Structure):
    """Mirror of ``asw_census_params`` (include/asw.h): window and the integer weights of
    ``w_a * min(AD, tau) + w_c * hamming``."""

    _fields_ = [("win_w", ctypes.c_int), ("win_h", ctypes.c_int), ("ad_weight", ctypes.c_int),
                ("census_weight", ctypes.c_int)]

    def copy(self) -> "AswCensusParams":
        return AswCensusParams(self.win_w, self.win_h, self.ad_weight, self.census_weight)


class AswSgmParams(ctypes.Structure):
    """Mirror of ``asw_sgm_params`` (include/asw.h): the number of paths (4 or 8) and the
    penalties ``0 <= p1 <= p2 <= 1048576`` of semi-global matching."""

    _fields_ = [("paths", ctypes.c_int), ("p1", ctypes.c_int), ("p2", ctypes.c_int)]

    def copy(self) -> "AswSgmParams":
        return AswSgmParams(self.paths, self.p1, self.p2)


class AswSpeckleParams(ctypes.Structure):
    """Mirror of ``asw_speckle_params`` (include/asw.h): the smallest component that is kept
    and the largest linked difference of the speckle filter."""

    _fields_ = [("min_size", ctypes.c_int), ("max_diff", ctypes.c_int)]

    def copy(self) -> "AswSpeckleParams":
        return AswSpeckleParams(self.min_size, self.max_diff)


class AswSpeckleOutputs(ctypes.Structure):
    """Mirror of ``asw_speckle_outputs``: caller-owned host [H][W] arrays, any may be NULL."""

    _fields_ = [("filtered16", ctypes.c_void_p), ("size", ctypes.c_void_p), ("keep", ctypes.c_void_p),
                ("disp_lr", ctypes.c_void_p), ("disp_filled", ctypes.c_void_p)]


SPECKLE_STATUS_OFFSET = 0  # ASW_SPECKLE_STATUS_OFFSET: the int32 status word of asw_speckle's workspace


class AswCrossTimings(ctypes.Structure):
    """Mirror of ``asw_cross_timings``: the reference's columns (main.cpp:394-410), ms."""

    _fields_ = [("median", ctypes.c_double * 2), ("cross", ctypes.c_double * 2)] + [
        (n, ctypes.c_double) for n in ("aggregation", "integral_h", "oii_h", "integral_v", "oii_v", "init", "vote",
                                       "total")]

    def as_dict(self) -> dict:
        d = {"median": list(self.median), "cross": list(self.cross)}
        d.update({n: getattr(self, n) for n, _ in self._fields_[2:]})
        return d


class AswCrossOutputs(ctypes.Structure):
    """Mirror of ``asw_cross_outputs``: caller-owned host arrays, any may be NULL."""

    _fields_ = [("initial_rgba", ctypes.c_void_p), ("final_rgba", ctypes.c_void_p),
                ("median_left_rgba", ctypes.c_void_p), ("d_initial", ctypes.c_void_p),
                ("timings", ctypes.POINTER(AswCrossTimings))]


class AswTimings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "raw_cost", "support", "v_pass_mean", "h_pass_mean", "aggregation_total", "wta",
        "consistency", "total", "h2d", "d2h", "refine", "exchange")]


_lib = None
_load_error: Exception | None = None

P = ctypes.c_void_p
PP = ctypes.POINTER(AswParams)
RP = ctypes.POINTER(AswRefineParams)
CP = ctypes.POINTER(AswCrossParams)
NP = ctypes.POINTER(AswCensusParams)
SP = ctypes.POINTER(AswSgmParams)
KP = ctypes.POINTER(AswSpeckleParams)
I = ctypes.c_int

# name -> (restype, argtypes).  Every function declared in include/asw.h.
SIGNATURES = {
    "asw_params_default": (None, [PP]),
    "asw_params_check": (I, [PP]),
    "asw_strerror": (ctypes.c_char_p, [I]),
    "asw_last_hip_error": (I, []),
    "asw_abi_version": (I, []),
    "asw_disp_pitch": (I, [PP]),
    "asw_tap_pitch": (I, [PP]),
    "asw_cost_bytes": (ctypes.c_size_t, [PP]),
    "asw_support_bytes": (ctypes.c_size_t, [PP]),
    "asw_lut_bytes": (ctypes.c_size_t, [PP]),
    "asw_raw_cost": (I, [PP, P, P, P, P]),
    "asw_support_lut": (I, [PP, P, P]),
    "asw_support": (I, [PP, I, P, P, P, P]),
    "asw_support_all": (I, [PP, P, P, P, P, P, P, P, P]),
    "asw_lab_bytes": (ctypes.c_size_t, [PP]),
    "asw_lab": (I, [PP, P, P, P]),
    "asw_support_lab": (I, [PP, I, P, P, P]),
    "asw_aggregate_pass": (I, [PP, I, P, P, P, P, P]),
    "asw_aggregate_pass_den": (I, [PP, I, P, P, P, P, P, I, P]),
    "asw_raw_cost16": (I, [PP, P, P, P, P]),
    "asw_aggregate_pass_den16": (I, [PP, P, P, P, P, P, I, P]),
    "asw_raw16_supported": (I, [PP]),
    "asw_aggregate": (I, [PP, P, P, P, P, P, P, P]),
    "asw_aggregate_den": (I, [PP, P, P, P, P, P, P, P, P, P]),
    "asw_wta": (I, [PP, P, P, P, P, P, P, P, P]),
    "asw_consistency": (I, [PP, P, P, P, P, P, P, P, P, P]),
    "asw_wta_local": (I, [PP, P, P, P, P, P]),
    "asw_wta_target_local": (I, [PP, P, P, P, P, P, P]),
    "asw_wta_second": (I, [PP, P, P, P, P, P, P]),
    "asw_wta_finalize": (I, [PP, P, P, P, P, P, P, P, P, P, P, P]),
    "asw_wta_ref_local": (I, [PP, P, P, P, P, P, P]),
    "asw_wta_ref_target_local": (I, [PP, P, P, P, P, P, P, P]),
    "asw_wta_ref_finalize": (I, [PP, P, P, P, P, P, P, P, P, P]),
    "asw_refine_params_default": (None, [RP]),
    "asw_refine_params_check": (I, [PP, RP]),
    "asw_refine_lut_bytes": (ctypes.c_size_t, [RP]),
    "asw_refine_lut": (I, [PP, RP, P, P]),
    "asw_ref_v": (I, [PP, RP, P, P, I, P, P, P, P]),
    "asw_ref_h": (I, [PP, RP, P, P, P, P, P, P]),
    "asw_wta_ref": (I, [PP, P, P, P, P, P, P, P, P, P]),
    "asw_median3": (I, [PP, P, I, P, P]),
    "asw_refine_workspace_bytes": (ctypes.c_size_t, [PP, RP]),
    "asw_refine": (I, [PP, RP, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "asw_set_refine": (I, [P, RP]),
    "asw_refine_native_params_check": (I, [PP, RP]),
    "asw_refine_native_lut": (I, [PP, RP, P, P]),
    "asw_ref_v_native": (I, [PP, RP, P, P, P, P, P, P]),
    "asw_consistency_native": (I, [PP, P, P, P, P, P, P, P]),
    "asw_median3_u16": (I, [PP, P, P, P]),
    "asw_refine_native_workspace_bytes": (ctypes.c_size_t, [PP, RP]),
    "asw_refine_native": (I, [PP, RP, P, P, P, P, P, P, P, P, P, P, P, P]),
    "asw_set_refine_native": (I, [P, RP, P]),
    "asw_set_graph": (I, [P, I]),
    "asw_subpixel": (I, [PP, P, P, P, P]),
    "asw_subpixel_local": (I, [PP, P, P, P, P]),
    "asw_subpixel_finalize": (I, [PP, P, P, P, P]),
    "asw_disp_mask": (I, [PP, P, P, P, P, P, P, P]),
    "asw_disp_fill": (I, [PP, P, P, P]),
    "asw_set_subpixel": (I, [P, P]),
    "asw_cross_params_default": (None, [CP]),
    "asw_cross_params_check": (I, [PP, CP]),
    "asw_cross_arm_bytes": (ctypes.c_size_t, [PP]),
    "asw_median3_rgba": (I, [PP, P, P, P]),
    "asw_cross_arms": (I, [PP, CP, P, P, P]),
    "asw_cross_cost": (I, [PP, P, P, P, P]),
    "asw_cross_integral": (I, [PP, I, P, P]),
    "asw_cross_oii": (I, [PP, I, P, P, P, P, P]),
    "asw_cross_init": (I, [PP, P, P, P, P]),
    "asw_cross_vote": (I, [PP, P, P, P, P, P]),
    "asw_set_cross": (I, [P, CP, ctypes.POINTER(AswCrossOutputs)]),
    "asw_census_params_default": (None, [NP]),
    "asw_census_params_check": (I, [PP, NP]),
    "asw_census_bytes": (ctypes.c_size_t, [PP]),
    "asw_census": (I, [PP, NP, P, P, P]),
    "asw_census_cost": (I, [PP, NP, P, P, P, P, P, P]),
    "asw_census_cost16": (I, [PP, NP, P, P, P, P, P, P]),
    "asw_census16_supported": (I, [PP, NP]),
    "asw_set_census": (I, [P, NP]),
    "asw_sgm_params_default": (None, [SP]),
    "asw_sgm_params_check": (I, [PP, SP]),
    "asw_sgm_workspace_bytes": (ctypes.c_size_t, [PP, SP]),
    "asw_sgm_path": (I, [PP, SP, I, P, P, I, P]),
    "asw_sgm": (I, [PP, SP, P, P, P, P]),
    "asw_set_sgm": (I, [P, SP]),
    "asw_speckle_params_default": (None, [KP]),
    "asw_speckle_params_check": (I, [PP, KP]),
    "asw_speckle_workspace_bytes": (ctypes.c_size_t, [PP]),
    "asw_lr_valid": (I, [PP, P, P, P, P, P, P]),
    "asw_speckle": (I, [PP, KP, P, P, P, P, P, P, P]),
    "asw_speckle_mask16": (I, [PP, P, P, P, P]),
    "asw_speckle_mask_f32": (I, [PP, P, P, P, P]),
    "asw_set_speckle": (I, [P, KP, ctypes.POINTER(AswSpeckleOutputs)]),
    "asw_tune_set": (I, [I, I]),
    "asw_pass_kernel": (I, [I, I, ctypes.c_char_p, I]),
    "asw_device_name": (I, [I, ctypes.c_char_p, I]),
    "asw_create": (I, [PP, I, ctypes.POINTER(P)]),
    "asw_destroy": (I, [P]),
    "asw_match": (I, [P, P, P, ctypes.POINTER(AswOutputs), ctypes.POINTER(AswTimings)]),
    "asw_create_multi": (I, [PP, ctypes.POINTER(I), I, ctypes.POINTER(P)]),
    "asw_comm_unique_id": (I, [ctypes.c_char_p]),
    "asw_create_rank": (I, [PP, I, I, I, ctypes.c_char_p, ctypes.POINTER(P)]),
    "asw_ctx_shard": (I, [P, I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)]),
    "asw_match_batch": (I, [P, P, P, I, ctypes.POINTER(AswOutputs), ctypes.POINTER(AswTimings)]),
}


def header_functions(path: str = HEADER_PATH) -> list[str]:
    """Names of every function the C header declares."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(asw_[a-z0-9_]+)\s*\(", text)) - {"asw_params", "asw_ctx"})


def _load():
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        _load_error = AswLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
        raise _load_error
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the environment
        _load_error = AswLibraryError(f"failed to load {LIB_PATH}: {e}")
        raise _load_error from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    got = L.asw_abi_version()
    if got != ABI_VERSION:
        _load_error = AswLibraryError(
            f"{LIB_PATH} has ABI revision {got}, this binding mirrors revision {ABI_VERSION} "
            "(asw_outputs / asw_timings layouts differ): rebuild the library")
        raise _load_error
    _lib = L
    return L


def _lib_or_raise():
    return _load()


def lib():
    return _load()


def strerror(status: int) -> str:
    return _load().asw_strerror(status).decode()


def check(status: int, where: str) -> None:
    if status != ASW_OK:
        raise AswError(status, where)


def default_params(width: int = 0, height: int = 0, **kw) -> AswParams:
    p = AswParams()
    _load().asw_params_default(ctypes.byref(p))
    p.width, p.height = width, height
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown asw_params field {k!r}")
        setattr(p, k, v)
    return p


def default_refine_params(**kw) -> AswRefineParams:
    """Reference refinement settings (k = 6, 33 taps, 10.94 / 118.78, 0.085), overridable."""
    rp = AswRefineParams()
    _load().asw_refine_params_default(ctypes.byref(rp))
    for k, v in kw.items():
        if not hasattr(rp, k):
            raise TypeError(f"unknown asw_refine_params field {k!r}")
        setattr(rp, k, v)
    return rp


def refine_is_native(p: AswParams, rp: AswRefineParams) -> bool:
    """True when (p, rp) needs the native refinement loop (asw_refine_native: indices and
    uint16 maps) because the 8-bit loop is not built for it (ndisp > 256, ASW_LR_NATIVE).
    Raises for a pair neither loop accepts."""
    L = _load()
    st = L.asw_refine_params_check(ctypes.byref(p), ctypes.byref(rp))
    if st == ASW_OK:
        return False
    check(L.asw_refine_native_params_check(ctypes.byref(p), ctypes.byref(rp)), "asw_refine_native_params_check")
    return True


def default_cross_params(**kw) -> AswCrossParams:
    """Reference settings of the cross-based matcher (arm_max 25, tau 25), overridable."""
    cp = AswCrossParams()
    _load().asw_cross_params_default(ctypes.byref(cp))
    for k, v in kw.items():
        if not hasattr(cp, k):
            raise TypeError(f"unknown asw_cross_params field {k!r}")
        setattr(cp, k, v)
    return cp


def default_census_params(**kw) -> AswCensusParams:
    """The default census cost (9 x 7 window, ad_weight 1, census_weight 8), overridable."""
    cp = AswCensusParams()
    _load().asw_census_params_default(ctypes.byref(cp))
    for k, v in kw.items():
        if not hasattr(cp, k):
            raise TypeError(f"unknown asw_census_params field {k!r}")
        setattr(cp, k, v)
    return cp


def census_params_of(census) -> AswCensusParams | None:
    """The ``census=`` keyword of the matchers: None / False (off), True (the defaults) or
    an AswCensusParams."""
    if census is None or census is False:
        return None
    return default_census_params() if census is True else census.copy()


def default_sgm_params(**kw) -> AswSgmParams:
    """The default semi-global matching parameters (8 paths, P1 16, P2 128), overridable."""
    sp = AswSgmParams()
    _load().asw_sgm_params_default(ctypes.byref(sp))
    for k, v in kw.items():
        if not hasattr(sp, k):
            raise TypeError(f"unknown asw_sgm_params field {k!r}")
        setattr(sp, k, v)
    return sp


def sgm_params_of(sgm) -> AswSgmParams | None:
    """The ``sgm=`` keyword of the matchers: None / False (off), True (the defaults) or an
    AswSgmParams."""
    if sgm is None or sgm is False:
        return None
    return default_sgm_params() if sgm is True else sgm.copy()


def default_speckle_params(**kw) -> AswSpeckleParams:
    """The default speckle filter (min_size 32, max_diff 1), overridable."""
    sp = AswSpeckleParams()
    _load().asw_speckle_params_default(ctypes.byref(sp))
    for k, v in kw.items():
        if not hasattr(sp, k):
            raise TypeError(f"unknown asw_speckle_params field {k!r}")
        setattr(sp, k, v)
    return sp


def speckle_params_of(speckle) -> AswSpeckleParams | None:
    """The ``speckle=`` keyword of the matchers: None / False (off), True (the defaults) or an
    AswSpeckleParams."""
    if speckle is None or speckle is False:
        return None
    return default_speckle_params() if speckle is True else speckle.copy()


def disp_pitch(p: AswParams) -> int:
    return _load().asw_disp_pitch(ctypes.byref(p))


def tap_pitch(p: AswParams) -> int:
    return _load().asw_tap_pitch(ctypes.byref(p))


def params_check(p: AswParams) -> int:
    return _load().asw_params_check(ctypes.byref(p))
