"""stereo_matchin_amd — MI355X-native adaptive-support-weight stereo matcher.

A drop-in for the OpenCL ``kernels/`` ASW path of manixq/stereo_matchin
(stereo_matching/main.cpp:413-537): hand-written gfx950 HIP kernels behind the
C-ABI in ``include/asw.h`` (``libasw_hip.so``), a Python mirror of the
reference's kernel interface (:mod:`.kernels`), the one-GPU pipeline
(:mod:`.pipeline`) and disparity-axis sharding over RCCL (:mod:`.distributed`).
"""
from ._lib import (ASW_OK, COLOR_LAB, COLOR_RGB, DIR_H, DIR_V, LR_NATIVE, LR_U8, AswError,  # noqa: F401
                   AswCensusParams, AswLibraryError, AswParams, AswSgmParams, AswSpeckleParams,
                   AswSubpixelOutputs, default_census_params, default_params, default_sgm_params,
                   default_speckle_params)
from .pipeline import (CrossMatcher, CrossResult, FrameContext, MatchResult, StereoMatcher,  # noqa: F401
                       comm_unique_id, make_params, match_frame, to_rgba)

__all__ = [
    "AswParams", "AswError", "AswLibraryError", "StereoMatcher", "MatchResult", "make_params", "match_frame",
    "FrameContext", "comm_unique_id", "CrossMatcher", "CrossResult",
    "to_rgba", "default_params", "AswSubpixelOutputs", "AswCensusParams", "default_census_params",
    "AswSgmParams", "default_sgm_params", "AswSpeckleParams", "default_speckle_params",
]
