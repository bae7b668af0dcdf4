"""ir2rgb_amd -- MI355X-native (gfx950) implementation of the ir2rgb vid2vid hot path.

Everything computational goes through ``lib/libir2rgb_hip.so`` (hand-written HIP, C ABI in
include/ir2rgb_hip.h).  Importing the package never touches the GPU; the library is loaded on
first use and its absence is an error (there is no CPU fallback).
"""
__version__ = "0.1.0"

__all__ = ["VideoTranslator", "VideoScore", "video_metrics", "ssim_reference", "warp_error", "warp_error_reference",
           "warp_bound", "colour_metrics", "colour_reference", "colour_bound", "srgb_table", "FrameScaler", "img_params", "resample_coeffs", "resize_reference", "TrainingSchedule", "LossLog", "fit", "Snapshots", "to_u8_reference", "flow_to_rgb_reference",
           "JpegEncoder", "jpeg_reference", "JpegDecoder", "decode_reference", "FolderSequences", "ThermalAGC", "agc_reference"]


def __getattr__(name):
    # resolved on first use: importing the package stays free of torch and of the GPU
    if name == "VideoTranslator":
        from .inference import VideoTranslator
        return VideoTranslator
    if name in ("VideoScore", "video_metrics", "ssim_reference", "warp_error", "warp_error_reference", "warp_bound",
                "colour_metrics", "colour_reference", "colour_bound", "srgb_table"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("FrameScaler", "img_params", "resample_coeffs", "resize_reference"):
        from . import transform
        return getattr(transform, name)
    if name in ("Snapshots", "to_u8_reference", "flow_to_rgb_reference"):
        from . import visuals
        return getattr(visuals, name)
    if name in ("JpegEncoder", "jpeg_reference"):
        from . import jpeg
        return getattr(jpeg, name)
    if name in ("JpegDecoder", "decode_reference"):
        from . import jpeg_decode
        return getattr(jpeg_decode, name)
    if name in ("ThermalAGC", "agc_reference"):
        from . import thermal
        return getattr(thermal, name)
    if name == "FolderSequences":
        from .frames import FolderSequences
        return FolderSequences
    if name == "TrainingSchedule":
        from .schedule import TrainingSchedule
        return TrainingSchedule
    if name == "LossLog":
        from .losslog import LossLog
        return LossLog
    if name == "fit":
        from .training import fit
        return fit
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
