"""MI355X-native render path for ccelio/TileCodeRayTracer.

The product is the C-ABI library ``lib/libtcrt.so`` (include/rt_capi.h):
hand-written HIP kernels for gfx950 behind "render every pixel of a
rectangle".  This package is the thin Python side used by the tests and by
bench.py: ctypes bindings to that library (:mod:`.capi`), bindings to the C++
host model that mirrors the reference's Scene / SceneObject / Camera API
(:mod:`.host`), and a small convenience wrapper (:mod:`.renderer`).

There is no CPU rendering path anywhere in this package; if the HIP library is
missing or no GPU is present, rendering raises.
"""
from .capi import RtError, load_library, library_path  # noqa: F401
from .host import HostScene  # noqa: F401
from .renderer import Renderer, adaptive_flags, denoise, encode_image, indirect_rays, lens_rays, subsample_hits, upsample_guided  # noqa: F401
from .renderer import TemporalHistory, temporal_accumulate, temporal_params  # noqa: F401
from .renderer import svgf_filter, svgf_params  # noqa: F401
from .renderer import motion_accumulate, object_motions, render_animated  # noqa: F401
from .renderer import mirror_params  # noqa: F401
from .renderer import glass_params  # noqa: F401
from .renderer import clamp_params, history_clamp  # noqa: F401
from .renderer import gradient_params, gradient_reweight  # noqa: F401
from .renderer import paths_params  # noqa: F401

__all__ = ["RtError", "load_library", "library_path", "HostScene", "Renderer", "adaptive_flags", "denoise", "encode_image",
           "indirect_rays", "lens_rays", "subsample_hits", "upsample_guided", "TemporalHistory", "temporal_accumulate",
           "temporal_params", "svgf_filter", "svgf_params", "motion_accumulate", "object_motions", "render_animated",
           "mirror_params", "glass_params", "clamp_params", "history_clamp",
           "gradient_params", "gradient_reweight", "paths_params"]
