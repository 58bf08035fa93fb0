"""The ASW sequence of main.cpp:463-537 on one GPU, over the HIP C-ABI.

:class:`StereoMatcher` owns the device buffers of one image size / parameter
set (the reference re-creates every ``cl_mem`` per run, main.cpp:243-457; here
they are allocated once and reused across frames) and runs

    asw_Aggr -> 4 x support -> r x (V pass, H pass) -> asw_WTA -> Constistency

on torch's current stream.  ``match()`` takes device-resident RGBA8 images.
:func:`match_frame` is the host-pointer frame API (``asw_match``) used by the
CLI path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import COLOR_LAB, DIR_H, DIR_V, AswParams


def make_params(width: int, height: int, ndisp: int = 61, taps: int = 33, iters: int = 7, **kw) -> AswParams:
    """asw_params with the reference defaults (include/asw.h) and the given overrides."""
    return _lib.default_params(width, height, ndisp=ndisp, taps=taps, iters=iters, **kw)


@dataclass
class MatchResult:
    d_ref: torch.Tensor       # int32 [H][W] left-view disparity index
    conf_ref: torch.Tensor    # float32 [H][W]
    d_tar: torch.Tensor       # int32 [H][W] right-view (target) index
    conf_tar: torch.Tensor
    code_ref: torch.Tensor    # u8 [H][W] 8-bit image codes (asw_left_wta)
    code_tar: torch.Tensor
    lr_rgba: torch.Tensor | None       # consistency_error
    lr_red_rgba: torch.Tensor | None   # consistency_error_red (asw_consistency_pre-reff.png)
    cost: torch.Tensor        # final aggregated volume [H][W][Dp]
    # sub-pixel float maps (match(..., subpixel=True)): float32 [H][W]
    disp: torch.Tensor | None = None         # d_ref + parabola offset of the neighbouring planes
    disp_lr: torch.Tensor | None = None      # disp where the LR check passes, NaN elsewhere
    disp_filled: torch.Tensor | None = None  # disp_lr with its holes filled per row
    # speckle filter (StereoMatcher(speckle=...)): connected components of d_ref under the LR rule
    speckle_keep: torch.Tensor | None = None  # uint8 [H][W]: valid and in a component of >= min_size pixels
    speckle_size: torch.Tensor | None = None  # int32 [H][W] component size, 0 where invalid
    filtered16: torch.Tensor | None = None    # uint16 in int16 storage: d_ref where kept, else 0xFFFF


class StereoMatcher:
    """One GPU, one disparity shard: the buffers of main.cpp:434-457, allocated once.

    ``den_cache`` (default on for r >= 2): keep the two aggregation denominators
    (V, H) as volumes — written by the first pass of each direction, read by the
    other r-1 (ASW_DEN_*); bit-identical results, 2 more cost-sized buffers.

    ``census``: None (the AD raw cost), True (the default AD-census cost) or an
    AswCensusParams: ``raw_and_support`` then runs asw_census on both images and the census
    cost in place of asw_Aggr (include/asw.h §census).

    ``sgm``: None (the ASW passes), True (8 paths, P1 16, P2 128) or an AswSgmParams:
    semi-global matching (asw_sgm) on the uint16 raw cost in place of the supports and the
    passes; ``taps`` and ``iters`` are then not read and no support array is allocated
    (include/asw.h §SGM).

    ``speckle``: None (off), True (min_size 32, max_diff 1) or an AswSpeckleParams: ``match``
    then runs the speckle filter (asw_speckle) on d_ref, valid where the LR check passes (every
    pixel without it), and fills ``speckle_keep`` / ``speckle_size`` / ``filtered16``."""

    def __init__(self, params: AswParams, device="cuda", den_cache: bool = True, census=None, sgm=None,
                 speckle=None):
        st = _lib.params_check(params)
        if st != _lib.ASW_OK:
            raise _lib.AswError(st, "asw_params_check")
        self.p = params.copy()
        self.census = _lib.census_params_of(census)
        if self.census is not None:
            _lib.check(_lib.lib().asw_census_params_check(ctypes.byref(self.p), ctypes.byref(self.census)),
                       "asw_census_params_check")
        self.sgm = _lib.sgm_params_of(sgm)
        self.speckle = _lib.speckle_params_of(speckle)
        if self.speckle is not None:
            _lib.check(_lib.lib().asw_speckle_params_check(ctypes.byref(self.p), ctypes.byref(self.speckle)),
                       "asw_speckle_params_check")
        self.device = torch.device(device)
        dev = self.device
        self.local = None
        if self.sgm is not None:
            _lib.check(_lib.lib().asw_sgm_params_check(ctypes.byref(self.p), ctypes.byref(self.sgm)),
                       "asw_sgm_params_check")
            self.cen_l = self.cen_r = None
            if self.census is not None:
                self.cen_l = torch.empty((self.p.height, self.p.width), dtype=torch.int64, device=dev)
                self.cen_r = torch.empty_like(self.cen_l)
            # the raw cost as uint16 in c1's first half, the sums in c0 (what match() reads on)
            self.c0 = K.new_cost(self.p, dev)
            self.c1 = K.new_cost(self.p, dev)
            self.raw16 = True
            self.c1_16 = K.cost16_view(self.c1)
            # what only the supports and the passes use
            self.lut = self.wvl = self.wvr = self.whl = self.whr = None
            self.c0_16 = self.den_v = self.den_h = None
            return
        self.lut = torch.empty(K.lut_shape(self.p), dtype=torch.float32, device=dev)
        self.wvl, self.wvr, self.whl, self.whr = (K.new_support(self.p, dev) for _ in range(4))
        self.c0 = K.new_cost(self.p, dev)
        self.c1 = K.new_cost(self.p, dev)
        # the raw costs as uint16 in c0's first half (asw_raw_cost16 + the first V pass
        # asw_aggregate_pass_den16: half the bytes of asw_Aggr's write and that pass's read,
        # bit-identical); ASW_FLAG_RAW_F32 keeps the float volume
        self.raw16 = not params.flags & _lib.FLAG_RAW_F32 and (
            K.raw16_supported(self.p) if self.census is None else K.census16_supported(self.p, self.census))
        self.cen_l = self.cen_r = None
        if self.census is not None:
            self.cen_l = torch.empty((self.p.height, self.p.width), dtype=torch.int64, device=dev)
            self.cen_r = torch.empty_like(self.cen_l)
        self.c0_16 = K.cost16_view(self.c0) if self.raw16 else None
        self.den_v = self.den_h = None
        if den_cache and self.p.iters >= 2 and K.cost_shape(self.p)[2] != 32:
            # a 32-plane shard's passes recompute den (C4 / 8: k_vpass32 den-none 0.24
            # against den-read 0.28 ms, k_hpass32 0.30-0.33 against 0.36,
            # profiles/r04/h32_variants_r11d.log; asw_frame.cpp the same)
            self.den_v = K.new_cost(self.p, dev)
            self.den_h = K.new_cost(self.p, dev)
        # the WTA's local scan (key, m1, m2) of c0 when a pass already produced it (None:
        # asw_WTA / asw_wta_local scan the volume); read by match() and the d-sharded protocol
        self.local = None

    # -- stages ---------------------------------------------------------------
    def raw_and_support(self, left: torch.Tensor, right: torch.Tensor):
        """asw_Aggr (or the census cost) into c0 and the four support arrays; with SGM on
        the uint16 raw cost into c1 alone."""
        p = self.p
        if self.sgm is not None:
            if self.census is not None:
                K.census(p, self.census, left, out=self.cen_l)
                K.census(p, self.census, right, out=self.cen_r)
                K.census_cost16(p, self.census, left, right, self.cen_l, self.cen_r, out=self.c1_16)
            else:
                K.asw_Aggr16(p, left, right, out=self.c1_16)
            return
        if self.census is not None:
            cp = self.census
            K.census(p, cp, left, out=self.cen_l)
            K.census(p, cp, right, out=self.cen_r)
            if self.raw16:
                K.census_cost16(p, cp, left, right, self.cen_l, self.cen_r, out=self.c0_16)
            else:
                K.census_cost(p, cp, left, right, self.cen_l, self.cen_r, out=self.c0)
        elif self.raw16:
            K.asw_Aggr16(p, left, right, out=self.c0_16)
        else:
            K.asw_Aggr(p, left, right, out=self.c0)
        if p.color_space == COLOR_LAB:
            lab_l, lab_r = K.lab_image(p, left), K.lab_image(p, right)
            K.support_lab(p, DIR_V, lab_l, out=self.wvl)
            K.support_lab(p, DIR_H, lab_l, out=self.whl)
            K.support_lab(p, DIR_V, lab_r, out=self.wvr)
            K.support_lab(p, DIR_H, lab_r, out=self.whr)
            return
        K.support_lut(p, self.device, out=self.lut)
        # asw_vSupport / asw_hSupport of both images (main.cpp:469-484) in one launch
        K.support_all(p, left, right, self.lut, self.wvl, self.whl, self.wvr, self.whr)

    def aggregate(self, events: list | None = None):
        """r x (V: c0 -> c1, H: c1 -> c0); the result is in c0 (main.cpp:486-515)."""
        p = self.p
        self.local = None
        if self.sgm is not None:  # asw_sgm: c1 (uint16 raw cost) -> c0
            K.sgm(p, self.sgm, self.c1_16, out=self.c0)
            if events is not None:
                events.append(("sgm", _record()))
            return self.c0
        for it in range(p.iters):
            dmv = _lib.DEN_NONE if self.den_v is None else (_lib.DEN_WRITE if it == 0 else _lib.DEN_READ)
            dm = _lib.DEN_NONE if self.den_h is None else (_lib.DEN_WRITE if it == 0 else _lib.DEN_READ)
            if it == 0 and self.raw16:
                K.asw_vCostAggregation16(p, self.wvl, self.wvr, self.c0_16, out=self.c1, den=self.den_v, den_mode=dmv)
            else:
                K.asw_vCostAggregation(p, self.wvl, self.wvr, self.c0, out=self.c1, den=self.den_v, den_mode=dmv)
            if events is not None:
                events.append(("v", _record()))
            K.asw_hCostAggregation(p, self.whl, self.whr, self.c1, out=self.c0, den=self.den_h, den_mode=dm)
            if events is not None:
                events.append(("h", _record()))
        return self.c0

    def match(self, left: torch.Tensor, right: torch.Tensor, lr_check: bool | None = None,
              events: list | None = None, subpixel: bool = False) -> MatchResult:
        """``subpixel``: also the float maps ``disp`` and, with the LR check, ``disp_lr`` /
        ``disp_filled`` (asw_subpixel, asw_disp_mask, asw_disp_fill)."""
        p = self.p
        if events is not None:
            events.append(("start", _record()))
        self.raw_and_support(left, right)
        if events is not None:
            events.append(("support", _record()))
        cost = self.aggregate(events)
        if self.local is not None:  # the own scan ran in the last pass: the target scan and finalize
            d_ref, conf_ref, d_tar, conf_tar, code_ref, code_tar = K.wta_from_local(p, cost, *self.local)
        else:
            d_ref, conf_ref, d_tar, conf_tar, code_ref, code_tar = K.asw_WTA(p, cost)
        if events is not None:
            events.append(("wta", _record()))
        lr = red = None
        if p.lr_check if lr_check is None else lr_check:
            lr, red = K.Constistency(p, d_ref, d_tar, code_ref, code_tar, conf_ref, conf_tar)
        if events is not None:
            events.append(("consistency", _record()))
        res = MatchResult(d_ref, conf_ref, d_tar, conf_tar, code_ref, code_tar, lr, red, cost)
        if subpixel:
            res.disp = K.subpixel(p, cost, d_ref)
            if lr is not None:
                res.disp_lr, res.disp_filled = subpixel_lr_maps(p, res)
        if self.speckle is not None:
            valid = K.lr_valid(p, d_ref, d_tar, code_ref, code_tar) if lr is not None else None
            _, res.speckle_size, res.speckle_keep = K.speckle(p, self.speckle, d_ref, valid, want=("size", "keep"))
            if p.ndisp <= 65535:
                res.filtered16 = K.speckle_mask16(p, d_ref, res.speckle_keep)
        return res

    def refine(self, res: MatchResult, left: torch.Tensor, right: torch.Tensor, rp=None) -> dict:
        """The refinement loop + median (main.cpp:540-623) after ``match`` (needs its LR
        check).  ``res``'s lr image, target codes and confidences are refined in place
        like the reference's buffers; returns post_red_rgba (asw_consistency_post-reff),
        final_rgba (asw_disparity.png) and the last asw_WTA_REF maps.

        Where the 8-bit loop is not built (ndisp > 256, ASW_LR_NATIVE) the native loop runs
        instead (asw_refine_native, on indices): ``res``'s confidences are refined in place,
        its maps stay; returns final16 / post16 (uint16 maps in int16 storage, 0xFFFF =
        inconsistent), the last asw_WTA_REF maps d_ref / d_tar and est_left."""
        if res.lr_rgba is None:
            raise ValueError("refinement starts from the consistency image: match() with lr_check")
        rp = _lib.default_refine_params() if rp is None else rp
        if _lib.refine_is_native(self.p, rp):
            est_left, _ = K.consistency_native(self.p, res.d_ref, res.d_tar)
            return K.refine_native(self.p, rp, left, right, res.cost, est_left, res.d_tar.clone(), res.conf_ref,
                                   res.conf_tar)
        return K.refine(self.p, rp, left, right, res.cost, res.lr_rgba, res.code_tar, res.conf_ref, res.conf_tar)


@dataclass
class CrossResult:
    median_l: torch.Tensor      # u8 [H][W][4] median.png
    arms_l: torch.Tensor        # int8 [H][W][4] (h-, h+, v-, v+)
    arms_r: torch.Tensor
    d_initial: torch.Tensor     # int32 [H][W]
    code_initial: torch.Tensor  # u8 [H][W] cross_based_initial.png grey values
    d_final: torch.Tensor       # int32 [H][W] the vote, before the final median
    code_final: torch.Tensor    # u8 [H][W]
    final_rgba: torch.Tensor    # u8 [H][W][4] cross_based_disparity.png


class CrossMatcher:
    """The reference's cross-based matcher (main.cpp:243-411) on one GPU, stage by stage on
    torch's current stream:

        Median x 2 -> Cross x 2 -> Aggregation -> Integral_h -> Oii_hcross -> Integral_v
        -> Oii_vcross -> Init_disparity -> Disparity -> Median

    It owns two cost volumes, allocated once."""

    def __init__(self, params: AswParams, device="cuda", cross_params=None):
        self.p = params.copy()
        self.cp = _lib.default_cross_params() if cross_params is None else cross_params
        st = _lib.lib().asw_cross_params_check(ctypes.byref(self.p), ctypes.byref(self.cp))
        if st != _lib.ASW_OK:
            raise _lib.AswError(st, "asw_cross_params_check")
        self.device = torch.device(device)
        self.c0 = K.new_cost(self.p, self.device)
        self.c1 = K.new_cost(self.p, self.device)

    def match(self, left: torch.Tensor, right: torch.Tensor) -> CrossResult:
        p, cp = self.p, self.cp
        med_l, med_r = K.Median_rgba(p, left), K.Median_rgba(p, right)
        arms_l, arms_r = K.Cross(p, cp, med_l), K.Cross(p, cp, med_r)
        K.Aggregation(p, med_l, med_r, out=self.c0)
        K.Integral(p, DIR_H, self.c0)
        K.Oii_cross(p, DIR_H, arms_l, arms_r, self.c0, out=self.c1)
        K.Integral(p, DIR_V, self.c1)
        K.Oii_cross(p, DIR_V, arms_l, arms_r, self.c1, out=self.c0)
        d0, code0 = K.Init_disparity(p, self.c0)
        d1, code1 = K.Disparity(p, code0, arms_l)
        return CrossResult(med_l, arms_l, arms_r, d0, code0, d1, code1, K.Median(p, code1))


def subpixel_lr_maps(p: AswParams, res: MatchResult):
    """(disp_lr, disp_filled) of a result that holds ``disp`` and went through the LR check."""
    disp_lr = K.disp_mask(p, res.disp, res.d_ref, res.d_tar, res.code_ref, res.code_tar)
    return disp_lr, K.disp_fill(p, disp_lr)


def _record():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def to_rgba(img: np.ndarray) -> np.ndarray:
    """RGB or RGBA u8 [H][W][C] -> contiguous RGBA8 (alpha 255), what lodepng::decode yields."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, axis=2)
    if img.shape[2] == 4:
        return np.ascontiguousarray(img)
    a = np.full(img.shape[:2] + (1,), 255, np.uint8)
    return np.ascontiguousarray(np.concatenate([img[..., :3], a], axis=2))


class FrameContext:
    """The FRAME API (``asw_create`` / ``asw_create_multi`` / ``asw_create_rank`` +
    ``asw_match`` / ``asw_match_batch``): host RGBA8 in, host maps out, buffers
    allocated once and reused pair after pair.

    ``devices``: HIP ordinals of the shards driven by this process (one = one GPU;
    several = the disparity range split across them, RCCL when distinct, a
    device-local reduction when an ordinal repeats).  ``rank``/``nranks``/``comm_id``:
    one process per GPU (``asw_create_rank``), ``comm_id`` from :func:`comm_unique_id`.
    """

    def __init__(self, params: AswParams, devices=(0,), rank: int | None = None, nranks: int | None = None,
                 comm_id: bytes | None = None, refine=None, graph: bool = False, census=None, sgm=None,
                 speckle=None):
        self.L = _lib.lib()
        self.p = params.copy()
        self.ctx = ctypes.c_void_p()
        devices = list(devices)
        if rank is not None:
            if len(devices) != 1 or comm_id is None or nranks is None:
                raise ValueError("rank mode: one device, nranks and comm_id")
            _lib.check(self.L.asw_create_rank(ctypes.byref(self.p), devices[0], rank, nranks, comm_id,
                                              ctypes.byref(self.ctx)), "asw_create_rank")
        elif len(devices) == 1:
            _lib.check(self.L.asw_create(ctypes.byref(self.p), devices[0], ctypes.byref(self.ctx)), "asw_create")
        else:
            arr = (ctypes.c_int * len(devices))(*devices)
            _lib.check(self.L.asw_create_multi(ctypes.byref(self.p), arr, len(devices), ctypes.byref(self.ctx)),
                       "asw_create_multi")
        self.cross = None  # set_cross: (AswCrossParams, want timings)
        # refine: an AswRefineParams, main.cpp:540-623 inside asw_match; where the 8-bit loop is
        # not built for the context (ndisp > 256, ASW_LR_NATIVE) the native loop on indices
        # (asw_set_refine_native), whose maps arrive as final16 / post16 / refine_d_ref / refine_d_tar
        self.refine_native = None
        if refine is not None and refine.iters > 0 and _lib.refine_is_native(self.p, refine):
            self.refine_native = _lib.AswRefineParams(refine.iters, refine.taps, refine.gamma_c, refine.gamma_g,
                                                      refine.alpha)
            # validated here with empty outputs; match_batch registers each call's arrays
            _lib.check(self.L.asw_set_refine_native(self.ctx, ctypes.byref(self.refine_native),
                                                    ctypes.byref(_lib.AswRefineNativeOutputs())),
                       "asw_set_refine_native")
            refine = None
        self.refine = refine is not None
        if refine is not None:
            _lib.check(self.L.asw_set_refine(self.ctx, ctypes.byref(refine)), "asw_set_refine")
        if graph:  # asw_set_graph: capture the device work into HIP graphs, replay them
            _lib.check(self.L.asw_set_graph(self.ctx, 1), "asw_set_graph")
        self.census = None
        if census is not None and census is not False:
            self.set_census(census)
        self.sgm = None
        if sgm is not None and sgm is not False:
            self.set_sgm(sgm)
        self.speckle = None
        if speckle is not None and speckle is not False:
            self.set_speckle(speckle)

    def set_speckle(self, speckle=True) -> None:
        """``asw_set_speckle``: the speckle filter (asw_speckle) on the pre-refinement d_ref of
        every later match, valid where the LR check passes (every pixel on a context without
        it).  Its results arrive under ``speckle_filtered16`` (ndisp <= 65535), ``speckle_size``
        and ``speckle_keep``, and with ``subpixel=True`` on a context with the LR check also
        ``speckle_disp_lr`` (NaN holes) and ``speckle_disp_filled``.  ``speckle``: an
        AswSpeckleParams, True for the defaults (min_size 32, max_diff 1), None / False to turn
        it off again."""
        sp = _lib.speckle_params_of(speckle)
        if sp is None:
            _lib.check(self.L.asw_set_speckle(self.ctx, None, None), "asw_set_speckle")
        else:  # validated here with empty outputs; match_batch registers each call's arrays
            _lib.check(self.L.asw_set_speckle(self.ctx, ctypes.byref(sp), ctypes.byref(_lib.AswSpeckleOutputs())),
                       "asw_set_speckle")
        self.speckle = sp

    def _speckle_outputs(self, B: int, subpixel: bool):
        H, W = self.p.height, self.p.width
        spk = {"speckle_size": np.empty((B, H, W), np.int32), "speckle_keep": np.empty((B, H, W), np.uint8)}
        if self.p.ndisp <= 65535:
            spk["speckle_filtered16"] = np.empty((B, H, W), np.uint16)
        if subpixel and self.p.lr_check:
            spk["speckle_disp_lr"] = np.empty((B, H, W), np.float32)
            spk["speckle_disp_filled"] = np.empty((B, H, W), np.float32)
        ko = _lib.AswSpeckleOutputs(**{k[len("speckle_"):]: v.ctypes.data for k, v in spk.items()})
        return spk, ko

    def set_sgm(self, sgm=True) -> None:
        """``asw_set_sgm``: semi-global matching (asw_sgm) on the uint16 raw cost in place of
        the supports and the ASW passes of every later match.  ``sgm``: an AswSgmParams, True
        for the defaults (8 paths, P1 16, P2 128), None / False to turn it off again.
        One-shard contexts whose cost has a uint16 form (else ASW_E_UNSUPPORTED)."""
        sp = _lib.sgm_params_of(sgm)
        _lib.check(self.L.asw_set_sgm(self.ctx, ctypes.byref(sp) if sp is not None else None), "asw_set_sgm")
        self.sgm = sp

    def set_census(self, census=True) -> None:
        """``asw_set_census``: the census / AD-census cost in place of the AD raw cost of every
        later match.  ``census``: an AswCensusParams, True for the defaults (9 x 7, AD + 8 x
        census), None / False to turn it off again.  Ranks of a multi-process frame must
        switch it alike."""
        cp = _lib.census_params_of(census)
        _lib.check(self.L.asw_set_census(self.ctx, ctypes.byref(cp) if cp is not None else None), "asw_set_census")
        self.census = cp

    def set_cross(self, cross_params=True, timings: bool = True) -> None:
        """``asw_set_cross``: run the cross-based matcher (main.cpp:243-411) ahead of the ASW
        stages of every later match; its results arrive under ``cross_initial_rgba``,
        ``cross_final_rgba``, ``cross_median_rgba``, ``cross_d_initial`` and
        ``cross_timings``.  ``cross_params``: an AswCrossParams, True for the reference
        values, None / False to turn it off again."""
        if cross_params is None or cross_params is False:
            _lib.check(self.L.asw_set_cross(self.ctx, None, None), "asw_set_cross")
            self.cross = None
            return
        cp = _lib.default_cross_params() if cross_params is True else cross_params
        # validated here with empty outputs; match_batch registers each call's arrays
        _lib.check(self.L.asw_set_cross(self.ctx, ctypes.byref(cp), ctypes.byref(_lib.AswCrossOutputs())),
                   "asw_set_cross")
        self.cross = (cp, timings)

    def _cross_outputs(self, B: int):
        H, W = self.p.height, self.p.width
        cr = {"cross_initial_rgba": np.empty((B, H, W, 4), np.uint8),
              "cross_final_rgba": np.empty((B, H, W, 4), np.uint8),
              "cross_median_rgba": np.empty((B, H, W, 4), np.uint8),
              "cross_d_initial": np.empty((B, H, W), np.int32)}
        tarr = (_lib.AswCrossTimings * B)() if self.cross[1] else None
        co = _lib.AswCrossOutputs(cr["cross_initial_rgba"].ctypes.data, cr["cross_final_rgba"].ctypes.data,
                                  cr["cross_median_rgba"].ctypes.data, cr["cross_d_initial"].ctypes.data,
                                  ctypes.cast(tarr, ctypes.POINTER(_lib.AswCrossTimings)) if tarr else None)
        return cr, tarr, co

    def shards(self) -> list[tuple[int, int]]:
        n, b, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.L.asw_ctx_shard(self.ctx, 0, ctypes.byref(n), None, None)
        out = []
        for i in range(n.value):
            _lib.check(self.L.asw_ctx_shard(self.ctx, i, None, ctypes.byref(b), ctypes.byref(e)), "asw_ctx_shard")
            out.append((b.value, e.value))
        return out

    def _outputs(self, want_cost: bool, want16: bool):
        H, W = self.p.height, self.p.width
        out = {
            "d_ref": np.empty((H, W), np.int32), "d_tar": np.empty((H, W), np.int32),
            "conf_ref": np.empty((H, W), np.float32), "conf_tar": np.empty((H, W), np.float32),
            "disp_rgba": np.empty((H, W, 4), np.uint8), "lr_rgba": np.empty((H, W, 4), np.uint8),
            "lr_red_rgba": np.empty((H, W, 4), np.uint8),
        }
        if want_cost:
            out["cost"] = np.zeros((H, W, _lib.disp_pitch(self.p)), np.float32)
        if self.refine:
            out["final_rgba"] = np.empty((H, W, 4), np.uint8)
            out["post_red_rgba"] = np.empty((H, W, 4), np.uint8)
        if want16:
            out["disp16"] = np.empty((H, W), np.uint16)
            out["lr16"] = np.empty((H, W), np.uint16)
        o = _lib.AswOutputs(*[out[k].ctypes.data if k in out else None for k, _ in _lib.AswOutputs._fields_])
        return out, o

    def match(self, left_rgba: np.ndarray, right_rgba: np.ndarray, want_cost: bool = False,
              want16: bool = False, subpixel: bool = False) -> dict:
        return self.match_batch(left_rgba[None], right_rgba[None], want_cost, want16, subpixel)[0]

    def match_batch(self, lefts: np.ndarray, rights: np.ndarray, want_cost: bool = False,
                    want16: bool = False, subpixel: bool = False) -> list[dict]:
        """``asw_match_batch``: lefts / rights are [B][H][W][4] (or RGB) stacks.
        ``subpixel``: also the float maps ``disp_sub`` and, on a context with the LR check,
        ``disp_sub_lr`` (NaN holes) / ``disp_sub_filled`` (asw_set_subpixel)."""
        H, W = self.p.height, self.p.width
        lefts = np.ascontiguousarray(np.stack([to_rgba(x) for x in lefts]))
        rights = np.ascontiguousarray(np.stack([to_rgba(x) for x in rights]))
        B = lefts.shape[0]
        assert lefts.shape == (B, H, W, 4) and rights.shape == (B, H, W, 4)
        outs, os_ = zip(*[self._outputs(want_cost, want16) for _ in range(B)]) if B else ((), ())
        oarr = (_lib.AswOutputs * B)(*os_)
        tarr = (_lib.AswTimings * B)()
        sub = {}
        if subpixel and B:
            names = ("disp_sub", "disp_sub_lr", "disp_sub_filled") if self.p.lr_check else ("disp_sub",)
            sub = {k: np.empty((B, H, W), np.float32) for k in names}
            so = _lib.AswSubpixelOutputs(*[sub[k].ctypes.data for k in names])
            _lib.check(self.L.asw_set_subpixel(self.ctx, ctypes.byref(so)), "asw_set_subpixel")
        cr, ctim = {}, None
        if self.cross is not None and B:
            cr, ctim, co = self._cross_outputs(B)
            _lib.check(self.L.asw_set_cross(self.ctx, ctypes.byref(self.cross[0]), ctypes.byref(co)), "asw_set_cross")
        nat = {}
        if self.refine_native is not None and B:
            nat = {"final16": np.empty((B, H, W), np.uint16), "post16": np.empty((B, H, W), np.uint16),
                   "refine_d_ref": np.empty((B, H, W), np.int32), "refine_d_tar": np.empty((B, H, W), np.int32)}
            no = _lib.AswRefineNativeOutputs(*[v.ctypes.data for v in nat.values()])
            _lib.check(self.L.asw_set_refine_native(self.ctx, ctypes.byref(self.refine_native), ctypes.byref(no)),
                       "asw_set_refine_native")
        spk = {}
        if self.speckle is not None and B:
            spk, ko = self._speckle_outputs(B, subpixel)
            _lib.check(self.L.asw_set_speckle(self.ctx, ctypes.byref(self.speckle), ctypes.byref(ko)),
                       "asw_set_speckle")
        try:
            _lib.check(self.L.asw_match_batch(self.ctx, lefts.ctypes.data, rights.ctypes.data, B, oarr, tarr),
                       "asw_match_batch")
        finally:
            if sub:  # the registered arrays are this call's: off again
                self.L.asw_set_subpixel(self.ctx, None)
            if nat:  # this call's arrays leave the context; the loop stays on
                self.L.asw_set_refine_native(self.ctx, ctypes.byref(self.refine_native),
                                             ctypes.byref(_lib.AswRefineNativeOutputs()))
            if cr:  # this call's arrays leave the context; the matcher stays on
                self.L.asw_set_cross(self.ctx, ctypes.byref(self.cross[0]), ctypes.byref(_lib.AswCrossOutputs()))
            if spk:  # this call's arrays leave the context; the filter stays on
                self.L.asw_set_speckle(self.ctx, ctypes.byref(self.speckle), ctypes.byref(_lib.AswSpeckleOutputs()))
        for k, v in {**sub, **cr, **nat, **spk}.items():
            for b in range(B):
                outs[b][k] = v[b]
        if ctim is not None:
            for b in range(B):
                outs[b]["cross_timings"] = ctim[b].as_dict()
        for b in range(B):
            outs[b]["timings"] = \
                {f: getattr(tarr[b], f) for f, _ in tarr[b]._fields_}
        return list(outs)

    def close(self):
        if self.ctx:
            self.L.asw_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """``asw_comm_unique_id`` (ncclGetUniqueId) for :class:`FrameContext` rank mode."""
    buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
    _lib.check(_lib.lib().asw_comm_unique_id(buf), "asw_comm_unique_id")
    return buf.raw


def match_frame(params: AswParams, left_rgba: np.ndarray, right_rgba: np.ndarray, device: int = 0,
                want_cost: bool = False, refine=None, devices=None, want16: bool = False, census=None,
                sgm=None, speckle=None) -> dict:
    """Frame API (``asw_create`` + ``asw_match``): host RGBA8 in, host maps out."""
    with FrameContext(params, devices=devices if devices is not None else (device,), refine=refine,
                      census=census, sgm=sgm, speckle=speckle) as fc:
        return fc.match(left_rgba, right_rgba, want_cost=want_cost, want16=want16)
