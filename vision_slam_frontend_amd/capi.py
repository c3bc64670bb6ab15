"""ctypes binding of the C ABI in include/vsf.h (libvsf_hip.so, gfx950 HIP kernels).

There is NO CPU fallback: if the shared library is missing or a GPU call fails this module raises.
Host-side conveniences only (numpy in / numpy out for the host-pointer entry points, raw device pointers
for the batched entry points, which callers fill from torch tensors).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libvsf_hip.so"
# The instances of the selection kernel (k_select.hip): threads, stage-1 entries kept in LDS, stage-2 pairs kept in LDS
SELECT_FORMS = {"A": (1024, 12288, 512), "B": (256, 3072, 512), "C": (256, 9216, 512), "D": (64, 1536, 512)}

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
VISION_FEATURE_DTYPE = np.dtype([("feature_idx", "<u8"), ("pixel", "<f4", (2,)), ("point3d", "<f4", (3,))])
FEATURE_MATCH_DTYPE = np.dtype([("feature_idx_initial", "<u8"), ("feature_idx_current", "<u8")])
assert VISION_FEATURE_DTYPE.itemsize == 28 and FEATURE_MATCH_DTYPE.itemsize == 16
DESC_BYTES = 32
PAYLOAD_MAGIC = 0x31465356  # "VSF1"

VSF_OK, VSF_ERR_INVALID_ARG, VSF_ERR_CAPACITY, VSF_ERR_HIP, VSF_ERR_UNSUPPORTED, VSF_ERR_NO_DEVICE = range(6)

# Every symbol include/vsf.h declares (tests check that the library exports all of them).
EXPORTS = [
    "vsf_params_default", "vsf_params_set_ratio", "vsf_create", "vsf_destroy", "vsf_status_string",
    "vsf_last_hip_error", "vsf_get_params", "vsf_set_stream", "vsf_sync", "vsf_level_info", "vsf_extract",
    "vsf_fast_detect", "vsf_knn2_hamming", "vsf_get_matches", "vsf_extract_pair", "vsf_get_matches_multi", "vsf_extract_batch_dev", "vsf_match_batch_dev",
    "vsf_stereo_batch_dev", "vsf_set_lanes", "vsf_set_pipeline", "vsf_set_blur_overlap", "vsf_set_fast_resident", "vsf_get_fast_resident", "vsf_remove_ambig_stereo_batch_dev", "vsf_feature_matches_batch_dev", "vsf_bayer_bg_to_gray_batch_dev", "vsf_debug_level_image", "vsf_debug_fast_candidates", "vsf_debug_fast_work", "vsf_debug_level_keypoints",
    "vsf_algorithmic_bytes_per_image", "vsf_pyramid_pixels", "vsf_profile_enable", "vsf_profile_read",
    "vsf_stage_name", "vsf_debug_retain_best", "vsf_debug_retain_best_form", "vsf_debug_sort_trim", "vsf_stereo_residuals_batch_dev", "vsf_stereo_thresholds_dev",
    "vsf_stereo_filter_batch_dev", "vsf_vision_features_batch_dev", "vsf_packed_outputs_capacity",
    "vsf_pack_outputs_dev", "vsf_observe_capacity", "vsf_observe_stereo", "vsf_observe_submit", "vsf_observe_collect", "vsf_observe_reset",
    "vsf_observe_configure", "vsf_observe_collect_view", "vsf_observe_stats", "vsf_observe_poll", "vsf_debug_jpeg_serial",
    "vsf_jpeg_decode_gray_batch", "vsf_png_decode_gray_batch", "vsf_imdecode_gray_batch", "vsf_tune_fast_resident", "vsf_set_option", "vsf_get_option", "vsf_debug_inject_hip_error", "vsf_comm_unique_id", "vsf_comm_create", "vsf_comm_destroy", "vsf_comm_info",
    "vsf_allgather_dev", "vsf_gather_payload_dev", "vsf_reserve", "vsf_set_input_event",
    "vsf_observe_set_debug_images", "vsf_observe_debug_view", "vsf_draw_canvases_dev", "vsf_draw_canvases",
    "vsf_observe_submit_compressed", "vsf_observe_stereo_compressed", "vsf_observe_set_compressed_cap",
    "vsf_observe_default_compressed_cap", "vsf_observe_compressed_slot_bytes", "vsf_observe_compressed_ring_bytes",
    "vsf_compressed_image_size", "vsf_observe_probe_compressed",
    "vsf_observe_set_debug_jpeg", "vsf_observe_debug_jpeg_view", "vsf_jpeg_encode_capacity", "vsf_jpeg_encode_batch_dev", "vsf_jpeg_encode", "vsf_debug_jpeg_encode_header",
    "vsf_png_encode_capacity", "vsf_png_encode_batch_dev", "vsf_png_encode", "vsf_debug_png_encode_header", "vsf_debug_png_encode_cpu", "vsf_observe_set_debug_png", "vsf_observe_debug_png_view",
    "vsf_observe_set_streams", "vsf_observe_submit_stream", "vsf_observe_submit_compressed_stream", "vsf_observe_reset_stream",
    "vsf_observe_submit_dev", "vsf_observe_device_ring_bytes",
    "vsf_world_points_batch_dev", "vsf_world_points", "vsf_observe_set_world_points", "vsf_observe_set_pose",
    "vsf_observe_world_points_view",
    "vsf_imdecode_bgr_batch", "vsf_jpeg_decode_bgr_batch", "vsf_png_decode_bgr_batch",
    "vsf_imdecode_reduced_gray_batch", "vsf_reduced_size", "vsf_observe_probe_compressed_reduced",
    "vsf_observe_submit_compressed_reduced", "vsf_observe_stereo_compressed_reduced",
    "vsf_observe_set_debug_seeds", "vsf_observe_set_stream_cam_to_robot",
    "vsf_resize_gray_batch_dev", "vsf_observe_set_input_size", "vsf_resize_gray",
    "vsf_debug_describe_form", "vsf_debug_level_room",
    "vsf_pixfmt_bytes_per_pixel", "vsf_pixfmt_from_encoding", "vsf_to_gray_batch_dev",
    "vsf_observe_submit_stream_pix", "vsf_observe_set_bayer_order", "vsf_to_gray",
    "vsf_to_bgr_batch_dev", "vsf_to_bgr", "vsf_bag_extract_batch",
    "vsf_mask_set", "vsf_mask_set_dev", "vsf_mask_clear", "vsf_mask_is_set", "vsf_mask_slot_bytes", "vsf_set_image_masks",
    "vsf_get_image_masks", "vsf_debug_mask_level", "vsf_observe_set_stream_masks",
]
MAX_MASKS = 64  # VSF_MAX_MASKS
NO_MASK = -1
# vsf_option (include/vsf.h)
(OPT_FAST_BOTH_MAX, OPT_SELECT_WIDE, OPT_PYRAMID_FEW, OPT_PYRAMID_CHAIN, OPT_PYRAMID_ROWS, OPT_SELECT_BIG_CLASS,
 OPT_PIPE_AFTER_FAST, OPT_PIPE_PRIORITY, OPT_OBSERVE_THREAD, OPT_PYRAMID_TAIL_MIN, OPT_OBSERVE_COPY_THREAD,
 OPT_FAST_EARLY_LEVELS, OPT_FAST_EARLY_FORM, OPT_BLUR_EARLY) = range(14)
STAGE_COUNT = 8
# vsf_observe_stats' values, in order (include/vsf.h)
OBSERVE_STATS = ("frames", "batches", "max_batch", "solo", "forced", "slot_waits", "depth", "bmax", "copy_ns", "launch_ns",
                 "wait_ns", "compressed", "ingest_commands", "compressed_bytes", "debug_jpeg_commands", "streams",
                 "multi_stream_batches", "device_frames", "device_commands", "device_ring_bytes",
                 "world_points_frames", "world_points_commands", "world_points_ring_bytes", "reduced_frames",
                 "seeded_colour_frames", "colour_commands", "resized_frames", "resize_commands", "resize_bytes",
                 "multi_size_batches", "pixfmt_frames", "pixfmt_commands", "pixfmt_bytes")
# pixel formats of raw frames (include/vsf.h; 2 .. 15 stay unknown)
PIX_MONO8, PIX_BAYER_RGGB8 = 0, 1
PIX_BAYER_GRBG8, PIX_BAYER_GBRG8, PIX_BAYER_BGGR8, PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8 = range(16, 23)


class VsfParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("edge_threshold", C.c_int32), ("first_level", C.c_int32), ("wta_k", C.c_int32),
                ("score_type", C.c_int32), ("patch_size", C.c_int32), ("fast_threshold", C.c_int32),
                ("blur_sse2", C.c_int32), ("fast_detector_threshold", C.c_int32), ("fast_detector_nms", C.c_int32),
                ("ratio_num", C.c_uint32), ("ratio_shift", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_images", C.c_int32), ("max_keypoints", C.c_int32), ("residual_order", C.c_int32)]


class VsfCalibration(C.Structure):
    """vsf_calibration: FrontendConfig's stereo calibration (slam_frontend.cc:565-644), row-major floats."""
    _fields_ = [("projection_left", C.c_float * 12), ("projection_right", C.c_float * 12),
                ("camera_matrix_left", C.c_float * 9), ("distortion_left", C.c_float * 5),
                ("fundamental", C.c_float * 9), ("triangulate_rows", C.c_int32)]

    def set(self, name: str, values) -> "VsfCalibration":
        arr = getattr(self, name)
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        assert len(v) == len(arr), name
        for i, x in enumerate(v):
            arr[i] = float(x)
        return self

    def get(self, name: str) -> np.ndarray:
        return np.array(list(getattr(self, name)), np.float32)


# vsf_draw_op (include/vsf.h): kind, x0, y0, x1 (a circle's radius), y1, colour bytes in canvas (B, G, R) order
DRAW_CIRCLE, DRAW_LINE = 0, 1
DRAW_OP_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("bgr", "u1", (4,))])
assert DRAW_OP_DTYPE.itemsize == 24


class VsfDevFrame(C.Structure):
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("left_pitch", C.c_size_t), ("right_pitch", C.c_size_t)]


def device_image(t, width: int, height: int, device: int):
    """(address, pitch) of a 2-D uint8 tensor of height x width on GPU `device` whose rows are dense (stride(1) == 1; any
    stride(0) >= width): what vsf_observe_submit_dev takes.  ValueError for anything else -- before any call into the library."""
    if not (hasattr(t, "data_ptr") and hasattr(t, "stride") and hasattr(t, "is_cuda")):
        raise ValueError("a device image is a torch tensor, not %s" % type(t).__name__)
    if str(t.dtype) != "torch.uint8":
        raise ValueError("a device image is torch.uint8, not %s" % t.dtype)
    if not t.is_cuda or (t.device.index or 0) != device:
        raise ValueError("a device image lives on GPU %d, not on %s" % (device, t.device))
    if t.dim() != 2 or tuple(t.shape) != (height, width):
        raise ValueError("a device image is %d x %d, not %s" % (height, width, tuple(t.shape)))
    if t.stride(1) != 1 or (height > 1 and t.stride(0) < width):
        raise ValueError("a device image has dense rows (stride(1) == 1, stride(0) >= width), not strides %s" % (tuple(t.stride()),))
    return int(t.data_ptr()), int(t.stride(0)) if height > 1 else max(int(t.stride(0)), width)


def device_image_pix(t, width: int, height: int, device: int, pixfmt: int):
    """device_image for any PIX_* format: packed colour is a (height, width, 3 or 4) torch.uint8 tensor whose pixels are dense
    (stride(2) == 1, stride(1) == bytes per pixel; any stride(0) >= width * bytes per pixel)."""
    bpp = {PIX_BGR8: 3, PIX_RGB8: 3, PIX_BGRA8: 4, PIX_RGBA8: 4}.get(pixfmt, 1)
    if bpp == 1:
        return device_image(t, width, height, device)
    if not (hasattr(t, "data_ptr") and hasattr(t, "stride") and hasattr(t, "is_cuda")):
        raise ValueError("a device image is a torch tensor, not %s" % type(t).__name__)
    if str(t.dtype) != "torch.uint8":
        raise ValueError("a device image is torch.uint8, not %s" % t.dtype)
    if not t.is_cuda or (t.device.index or 0) != device:
        raise ValueError("a device image lives on GPU %d, not on %s" % (device, t.device))
    if t.dim() != 3 or tuple(t.shape) != (height, width, bpp):
        raise ValueError("a device image of this format is %d x %d x %d, not %s" % (height, width, bpp, tuple(t.shape)))
    if t.stride(2) != 1 or t.stride(1) != bpp or (height > 1 and t.stride(0) < width * bpp):
        raise ValueError("a colour device image has dense pixels and rows, not strides %s" % (tuple(t.stride()),))
    return int(t.data_ptr()), int(t.stride(0)) if height > 1 else max(int(t.stride(0)), width * bpp)


class VsfDrawCanvas(C.Structure):
    """vsf_draw_canvas: GRAY2BGR of src0 (and src1 to its right) with ops[op_begin, op_begin + op_count) drawn on it."""
    _fields_ = [("src0", C.c_void_p), ("src1", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("src_pitch", C.c_int64), ("out", C.c_void_p), ("out_pitch", C.c_int64), ("op_begin", C.c_int32),
                ("op_count", C.c_int32)]


class VsfError(RuntimeError):
    def __init__(self, status: int, where: str, hip: int = 0):
        self.status = status
        msg = "%s: %s" % (where, lib().vsf_status_string(status).decode())
        if status == VSF_ERR_HIP:
            msg += " (hipError %d)" % hip
        super().__init__(msg)


_lib = None


def reduced_size(width: int, height: int, reduce: int):
    """vsf_reduced_size: (status, width, height) of a width x height image after IMREAD_REDUCED_GRAYSCALE_<reduce>
    (ceil(width / reduce), ceil(height / reduce); reduce in 1, 2, 4, 8).  No context, no device."""
    w, h = C.c_int(0), C.c_int(0)
    st = lib().vsf_reduced_size(width, height, reduce, C.byref(w), C.byref(h))
    return st, int(w.value), int(h.value)


def pixfmt_bytes_per_pixel(pixfmt: int) -> int:
    """vsf_pixfmt_bytes_per_pixel: 1, 3 or 4; 0 for an unknown code.  No context, no device."""
    return int(lib().vsf_pixfmt_bytes_per_pixel(pixfmt))


def pixfmt_from_encoding(encoding: str):
    """vsf_pixfmt_from_encoding: (status, PIX_* code or None) of a sensor_msgs/Image encoding.  No context, no device."""
    code = C.c_int(-1)
    st = lib().vsf_pixfmt_from_encoding(encoding.encode(), C.byref(code))
    return st, (int(code.value) if st == VSF_OK else None)


def probe_compressed_reduced(data: bytes, reduce: int, width: int, height: int, cap_per_image: int, force_serial: bool = False):
    """vsf_observe_probe_compressed_reduced: (status, kind) -- what a reduced submit makes of ONE payload on the host."""
    b = np.frombuffer(bytes(data), np.uint8)
    kind = C.c_int(0)
    st = lib().vsf_observe_probe_compressed_reduced(_p(b), len(b), reduce, width, height, cap_per_image, int(force_serial),
                                                    C.byref(kind))
    return st, int(kind.value)


def jpeg_encode_capacity(width: int, height: int, channels: int) -> int:
    """Bytes that hold the JPEG file of any width x height x channels image (vsf_jpeg_encode_capacity)."""
    return int(lib().vsf_jpeg_encode_capacity(width, height, channels))


def jpeg_encode_header(width: int, height: int, channels: int, quality: int = 0) -> bytes:
    """The encoder's host half: SOI .. SOS header."""
    buf = np.zeros(640, np.uint8)
    n = C.c_size_t()
    st = lib().vsf_debug_jpeg_encode_header(width, height, channels, quality, buf.ctypes.data_as(C.c_void_p), 640, C.byref(n))
    if st != VSF_OK:
        raise VsfError(st, "vsf_debug_jpeg_encode_header")
    return buf[:n.value].tobytes()


def png_encode_capacity(width: int, height: int, channels: int) -> int:
    """Bytes that hold the PNG file of any width x height x channels image (vsf_png_encode_capacity)."""
    return int(lib().vsf_png_encode_capacity(width, height, channels))


def png_encode_header(width: int, height: int, channels: int) -> bytes:
    """The PNG encoder's host half: signature + IHDR (33 bytes), then the zlib stream's two header bytes."""
    buf = np.zeros(64, np.uint8)
    n = C.c_size_t()
    st = lib().vsf_debug_png_encode_header(width, height, channels, buf.ctypes.data_as(C.c_void_p), 64, C.byref(n))
    if st != VSF_OK:
        raise VsfError(st, "vsf_debug_png_encode_header")
    return buf[:n.value].tobytes()


def png_encode_cpu(img) -> bytes:
    """cv::imencode(".png", img) by the encoder's CPU model (vsf_debug_png_encode_cpu): (h, w) gray or (h, w, 3) BGR uint8."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    cap = png_encode_capacity(w, h, ch)
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t()
    st = lib().vsf_debug_png_encode_cpu(_p(img), w, h, ch, w * ch, _p(out), cap, C.byref(n))
    if st != VSF_OK:
        raise VsfError(st, "vsf_debug_png_encode_cpu")
    return out[:n.value].tobytes()


def lib() -> C.CDLL:
    """Loads libvsf_hip.so; raises (loudly) if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). The product has no CPU fallback." % LIB_PATH)
        L = C.CDLL(str(LIB_PATH))
        vp, i32, sz, pp = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(VsfParams)
        ip = C.POINTER(C.c_int)
        L.vsf_params_default.argtypes = [pp, i32, i32, i32]
        L.vsf_params_set_ratio.argtypes = [pp, C.c_float]
        L.vsf_create.argtypes = [pp, i32, C.POINTER(vp)]
        L.vsf_destroy.argtypes = [vp]
        L.vsf_destroy.restype = None
        L.vsf_status_string.argtypes = [i32]
        L.vsf_status_string.restype = C.c_char_p
        L.vsf_last_hip_error.argtypes = [vp]
        L.vsf_get_params.argtypes = [vp, pp]
        L.vsf_set_stream.argtypes = [vp, vp]
        L.vsf_sync.argtypes = [vp]
        L.vsf_level_info.argtypes = [vp, i32, ip, ip, C.POINTER(C.c_float), ip]
        L.vsf_extract.argtypes = [vp, vp, i32, i32, sz, vp, vp, i32, ip]
        L.vsf_fast_detect.argtypes = [vp, vp, i32, i32, sz, i32, i32, vp, i32, ip]
        L.vsf_extract_pair.argtypes = [vp, vp, vp, i32, i32, sz, vp, vp, ip, vp, vp, ip, i32]
        L.vsf_get_matches_multi.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, vp]
        L.vsf_knn2_hamming.argtypes = [vp, vp, i32, vp, i32, vp, vp]
        L.vsf_get_matches.argtypes = [vp, vp, i32, vp, i32, vp, i32, ip]
        L.vsf_extract_batch_dev.argtypes = [vp, vp, i32, sz, sz, vp, vp, vp]
        L.vsf_match_batch_dev.argtypes = [vp, vp, vp, sz, vp, vp, i32, vp, vp, vp, vp]
        L.vsf_stereo_batch_dev.argtypes = [vp, vp, i32, sz, sz, vp, vp, vp, vp, vp]
        L.vsf_set_lanes.argtypes = [vp, i32]
        L.vsf_set_pipeline.argtypes = [vp, i32]
        L.vsf_set_input_event.argtypes = [vp, vp]
        L.vsf_reserve.argtypes = [vp, i32, i32]
        L.vsf_set_blur_overlap.argtypes = [vp, i32]
        L.vsf_set_fast_resident.argtypes = [vp, i32]
        L.vsf_mask_set.argtypes = [vp, i32, vp, i32, i32, sz]
        L.vsf_mask_set_dev.argtypes = [vp, i32, vp, i32, i32, sz]
        L.vsf_mask_clear.argtypes = [vp, i32]
        L.vsf_mask_is_set.argtypes = [vp, i32, ip]
        L.vsf_mask_slot_bytes.argtypes = [vp, C.POINTER(sz)]
        L.vsf_set_image_masks.argtypes = [vp, i32, i32]
        L.vsf_get_image_masks.argtypes = [vp, ip, ip]
        L.vsf_debug_mask_level.argtypes = [vp, i32, i32, vp, sz]
        L.vsf_observe_set_stream_masks.argtypes = [vp, i32, i32, i32]
        L.vsf_get_fast_resident.argtypes = [vp, C.POINTER(C.c_int)]
        L.vsf_tune_fast_resident.argtypes = [vp, vp, i32, sz, sz, vp, vp, vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.vsf_set_option.argtypes = [vp, i32, i32]
        L.vsf_get_option.argtypes = [vp, i32, ip]
        L.vsf_debug_inject_hip_error.argtypes = [vp, i32]
        L.vsf_comm_unique_id.argtypes = [vp]
        L.vsf_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
        L.vsf_comm_destroy.argtypes = [vp]
        L.vsf_comm_destroy.restype = None
        L.vsf_comm_info.argtypes = [vp, ip, ip, ip]
        L.vsf_allgather_dev.argtypes = [vp, vp, vp, vp, sz]
        L.vsf_gather_payload_dev.argtypes = [vp, vp, vp, sz, vp, sz, i32]
        L.vsf_remove_ambig_stereo_batch_dev.argtypes = [vp, vp, vp, vp, vp, i32, vp, C.c_float, vp, vp, vp, vp, vp, vp]
        L.vsf_feature_matches_batch_dev.argtypes = [vp, vp, vp, sz, vp, vp, i32, C.c_float, vp, vp]
        L.vsf_bayer_bg_to_gray_batch_dev.argtypes = [vp, vp, i32, i32, i32, sz, sz, vp, sz, sz]
        L.vsf_to_gray_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, sz]
        L.vsf_to_gray.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, sz]
        L.vsf_to_bgr_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, sz]
        L.vsf_to_bgr.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, sz]
        L.vsf_bag_extract_batch.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]
        L.vsf_pixfmt_bytes_per_pixel.argtypes = [i32]
        L.vsf_pixfmt_bytes_per_pixel.restype = C.c_int
        L.vsf_pixfmt_from_encoding.argtypes = [C.c_char_p, ip]
        L.vsf_jpeg_encode_capacity.argtypes = [i32, i32, i32]
        L.vsf_jpeg_encode_capacity.restype = sz
        L.vsf_jpeg_encode_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, i32, vp, sz, vp]
        L.vsf_jpeg_encode.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, i32, vp, sz, vp]
        L.vsf_debug_jpeg_encode_header.argtypes = [i32, i32, i32, i32, vp, sz, C.POINTER(sz)]
        L.vsf_png_encode_capacity.argtypes = [i32, i32, i32]
        L.vsf_png_encode_capacity.restype = sz
        L.vsf_png_encode_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, vp]
        L.vsf_png_encode.argtypes = [vp, vp, i32, i32, i32, i32, sz, sz, vp, sz, vp]
        L.vsf_debug_png_encode_header.argtypes = [i32, i32, i32, vp, sz, C.POINTER(sz)]
        L.vsf_debug_png_encode_cpu.argtypes = [vp, i32, i32, i32, sz, vp, sz, C.POINTER(sz)]
        L.vsf_stereo_residuals_batch_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp]
        L.vsf_stereo_thresholds_dev.argtypes = [vp, vp, i32, vp, vp]
        L.vsf_stereo_filter_batch_dev.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.vsf_vision_features_batch_dev.argtypes = [vp, C.POINTER(VsfCalibration), vp, vp, vp, i32, vp, vp, vp]
        L.vsf_world_points_batch_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
        L.vsf_world_points.argtypes = [vp, vp, i32, vp, vp, vp, i32, ip]
        L.vsf_observe_set_world_points.argtypes = [vp, i32, vp]
        L.vsf_observe_set_pose.argtypes = [vp, i32, vp, vp]
        L.vsf_observe_world_points_view.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(i32)]
        L.vsf_packed_outputs_capacity.argtypes = [vp, i32, i32]
        L.vsf_packed_outputs_capacity.restype = sz
        L.vsf_pack_outputs_dev.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, sz]
        L.vsf_debug_sort_trim.argtypes = [vp, vp, i32, i32, C.c_float, i32, vp, vp]
        L.vsf_observe_capacity.argtypes = [vp, i32]
        L.vsf_observe_capacity.restype = sz
        L.vsf_observe_submit.argtypes = [vp, vp, vp, i32, i32, sz, C.POINTER(VsfCalibration), C.c_float, i32,
                                         C.POINTER(C.c_int64)]
        L.vsf_observe_collect.argtypes = [vp, C.c_int64, vp, sz, C.POINTER(sz)]
        L.vsf_observe_collect_view.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(sz)]
        L.vsf_observe_configure.argtypes = [vp, i32, i32, i32]
        L.vsf_observe_stats.argtypes = [vp, vp, i32]
        L.vsf_observe_poll.argtypes = [vp, C.c_int64, C.POINTER(i32)]
        L.vsf_observe_stereo.argtypes = [vp, vp, vp, i32, i32, sz, C.POINTER(VsfCalibration), C.c_float, i32, vp, sz,
                                         C.POINTER(sz)]
        L.vsf_observe_reset.argtypes = [vp]
        L.vsf_observe_set_streams.argtypes = [vp, i32]
        L.vsf_observe_reset_stream.argtypes = [vp, i32]
        L.vsf_observe_set_input_size.argtypes = [vp, i32, i32, i32]
        L.vsf_resize_gray_batch_dev.argtypes = [vp, vp, i32, i32, i32, sz, sz, vp, i32, i32, sz, sz]
        L.vsf_resize_gray.argtypes = [vp, vp, i32, i32, i32, sz, sz, vp, i32, i32, sz, sz]
        L.vsf_observe_submit_stream.argtypes = [vp, i32, vp, vp, i32, i32, sz, C.POINTER(VsfCalibration), C.c_float, i32,
                                                C.POINTER(C.c_int64)]
        L.vsf_observe_submit_stream_pix.argtypes = [vp, i32, vp, vp, i32, i32, sz, i32, C.POINTER(VsfCalibration), C.c_float, i32,
                                                    C.POINTER(C.c_int64)]
        L.vsf_observe_set_bayer_order.argtypes = [vp, i32, i32]
        L.vsf_observe_submit_compressed_stream.argtypes = [vp, i32, vp, sz, vp, sz, i32, C.POINTER(VsfCalibration), C.c_float,
                                                           i32, C.POINTER(C.c_int64)]
        L.vsf_observe_submit_dev.argtypes = [vp, i32, C.POINTER(VsfDevFrame), i32, i32, vp, C.POINTER(VsfCalibration), C.c_float,
                                             i32, C.POINTER(C.c_int64)]
        L.vsf_observe_device_ring_bytes.argtypes = [vp, i32]
        L.vsf_observe_device_ring_bytes.restype = sz
        L.vsf_observe_submit_compressed.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(VsfCalibration), C.c_float, i32,
                                                    C.POINTER(C.c_int64)]
        L.vsf_observe_stereo_compressed.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(VsfCalibration), C.c_float, i32, vp,
                                                    sz, C.POINTER(sz)]
        L.vsf_observe_set_compressed_cap.argtypes = [vp, sz]
        L.vsf_observe_default_compressed_cap.argtypes = [i32, i32]
        L.vsf_observe_default_compressed_cap.restype = sz
        L.vsf_observe_compressed_slot_bytes.argtypes = [sz]
        L.vsf_observe_compressed_slot_bytes.restype = sz
        L.vsf_observe_compressed_ring_bytes.argtypes = [i32, sz]
        L.vsf_observe_compressed_ring_bytes.restype = sz
        L.vsf_compressed_image_size.argtypes = [vp, sz, ip, ip]
        L.vsf_observe_probe_compressed.argtypes = [vp, sz, i32, i32, sz, i32, ip]
        L.vsf_observe_set_debug_images.argtypes = [vp, i32]
        L.vsf_observe_debug_view.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(vp)]
        L.vsf_observe_set_debug_jpeg.argtypes = [vp, i32]
        L.vsf_observe_set_debug_seeds.argtypes = [vp, vp, i32]
        L.vsf_observe_set_stream_cam_to_robot.argtypes = [vp, i32, vp]
        L.vsf_observe_debug_jpeg_view.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
        L.vsf_observe_set_debug_png.argtypes = [vp, i32]
        L.vsf_observe_debug_png_view.argtypes = [vp, C.c_int64, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
        L.vsf_draw_canvases_dev.argtypes = [vp, C.POINTER(VsfDrawCanvas), i32, vp, i32]
        L.vsf_draw_canvases.argtypes = [vp, C.POINTER(VsfDrawCanvas), i32, vp, i32]
        L.vsf_jpeg_decode_gray_batch.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, sz]
        L.vsf_png_decode_gray_batch.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, sz]
        L.vsf_imdecode_gray_batch.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, sz]
        for f in (L.vsf_imdecode_bgr_batch, L.vsf_jpeg_decode_bgr_batch, L.vsf_png_decode_bgr_batch):
            f.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, sz]
        L.vsf_imdecode_reduced_gray_batch.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, sz, sz]
        L.vsf_reduced_size.argtypes = [i32, i32, i32, ip, ip]
        L.vsf_observe_probe_compressed_reduced.argtypes = [vp, sz, i32, i32, i32, sz, i32, ip]
        L.vsf_observe_submit_compressed_reduced.argtypes = [vp, i32, vp, sz, vp, sz, i32, C.POINTER(VsfCalibration), C.c_float,
                                                            i32, C.POINTER(C.c_int64)]
        L.vsf_observe_stereo_compressed_reduced.argtypes = [vp, vp, sz, vp, sz, i32, C.POINTER(VsfCalibration), C.c_float, i32,
                                                            vp, sz, C.POINTER(sz)]
        L.vsf_debug_level_image.argtypes = [vp, i32, i32, i32, vp, sz]
        L.vsf_debug_fast_candidates.argtypes = [vp, i32, i32, vp, i32, ip]
        L.vsf_debug_fast_work.argtypes = [vp, i32, i32, vp, i32, ip, ip, vp, i32]
        L.vsf_debug_level_keypoints.argtypes = [vp, i32, i32, vp, i32, ip]
        L.vsf_debug_level_room.argtypes = [vp, vp, vp, i32, vp]
        L.vsf_debug_describe_form.argtypes = [vp, i32]
        L.vsf_algorithmic_bytes_per_image.argtypes = [vp]
        L.vsf_algorithmic_bytes_per_image.restype = C.c_uint64
        L.vsf_pyramid_pixels.argtypes = [vp]
        L.vsf_pyramid_pixels.restype = C.c_uint64
        L.vsf_debug_retain_best.argtypes = [vp, vp, vp, i32, i32, i32, i32, ip]
        L.vsf_debug_retain_best_form.argtypes = [vp, i32, i32, vp, vp, i32, i32, i32, ip]
        L.vsf_profile_enable.argtypes = [vp, i32]
        L.vsf_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]
        L.vsf_stage_name.argtypes = [i32]
        L.vsf_stage_name.restype = C.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(int(a) if a else 0)


def default_params(width: int, height: int, max_images: int = 2, nfeatures: int = 10000, **over) -> VsfParams:
    p = VsfParams()
    st = lib().vsf_params_default(C.byref(p), width, height, max_images)
    if st != VSF_OK:
        raise VsfError(st, "vsf_params_default")
    p.nfeatures = nfeatures
    ratio = over.pop("nn_match_ratio", None)
    if ratio is not None:
        st = lib().vsf_params_set_ratio(C.byref(p), ratio)
        if st != VSF_OK:
            raise VsfError(st, "vsf_params_set_ratio")
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


HARRIS_SCORE, FAST_SCORE = 0, 1  # vsf_params::score_type (cv::ORB::HARRIS_SCORE / FAST_SCORE)


def level_room(params: VsfParams):
    """vsf_debug_level_room (host only): (room per level, n_l per level, records per image) vsf_create would give `params`."""
    room = np.zeros(params.nlevels, np.int32)
    nfeat = np.zeros(params.nlevels, np.int32)
    total = C.c_int64()
    st = lib().vsf_debug_level_room(C.byref(params), _p(room), _p(nfeat), params.nlevels, C.byref(total))
    if st != VSF_OK:
        raise VsfError(st, "vsf_debug_level_room")
    return room, nfeat, int(total.value)


class Context:
    """One GPU's vsf_ctx.  Not thread-safe (same contract as the C ABI)."""

    def __init__(self, params: VsfParams, device: int = 0):
        self._h = C.c_void_p()
        st = lib().vsf_create(C.byref(params), device, C.byref(self._h))
        if st != VSF_OK:
            self._h = None
            raise VsfError(st, "vsf_create")
        self.params = VsfParams()
        lib().vsf_get_params(self._h, C.byref(self.params))
        self.device = device
        self._input_sizes = {}  # observe_set_input_size: what observe_submit_dev checks its tensors against
        self._n_streams = 1

    def close(self):
        if getattr(self, "_h", None):
            lib().vsf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except TypeError:  # interpreter shutdown: the module's globals are gone already (the process ends anyway)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st: int, where: str, allow_capacity: bool = False):
        if st == VSF_OK or (allow_capacity and st == VSF_ERR_CAPACITY):
            return st
        raise VsfError(st, where, lib().vsf_last_hip_error(self._h))

    # ---- geometry ----
    @property
    def nlevels(self) -> int:
        return self.params.nlevels

    def level_info(self, level: int):
        w, h, n, s = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        self._check(lib().vsf_level_info(self._h, level, C.byref(w), C.byref(h), C.byref(s), C.byref(n)),
                    "vsf_level_info")
        return w.value, h.value, s.value, n.value

    def algorithmic_bytes_per_image(self) -> int:
        return int(lib().vsf_algorithmic_bytes_per_image(self._h))

    def pyramid_pixels(self) -> int:
        return int(lib().vsf_pyramid_pixels(self._h))

    def set_stream(self, hip_stream: int | None):
        self._check(lib().vsf_set_stream(self._h, C.c_void_p(hip_stream or 0)), "vsf_set_stream")

    def set_lanes(self, lanes: int):
        self._check(lib().vsf_set_lanes(self._h, lanes), "vsf_set_lanes")

    def set_blur_overlap(self, on: bool):
        self._check(lib().vsf_set_blur_overlap(self._h, int(on)), "vsf_set_blur_overlap")

    def set_fast_resident(self, waves: int):
        """-1 (default): what tune_fast_resident measured for the batch size, the grid form otherwise; 0: FAST as one
        workgroup per four cells; 2..4: resident, that many waves per SIMD."""
        self._check(lib().vsf_set_fast_resident(self._h, int(waves)), "vsf_set_fast_resident")

    def tune_fast_resident(self, d_imgs: int, n_images: int, image_stride: int, row_stride: int, d_kp: int, d_desc: int,
                           d_counts: int, samples: int = 3):
        """vsf_tune_fast_resident: BLOCKING; returns (median ms of the grid form, median ms of the resident form)."""
        g, r = C.c_float(), C.c_float()
        self._check(lib().vsf_tune_fast_resident(self._h, C.c_void_p(d_imgs), n_images, image_stride, row_stride,
                                                 C.c_void_p(d_kp), C.c_void_p(d_desc), C.c_void_p(d_counts), samples,
                                                 C.byref(g), C.byref(r)), "vsf_tune_fast_resident")
        return g.value, r.value

    def set_option(self, option: int, value: int):
        self._check(lib().vsf_set_option(self._h, int(option), int(value)), "vsf_set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int()
        self._check(lib().vsf_get_option(self._h, int(option), C.byref(v)), "vsf_get_option")
        return v.value

    def get_fast_resident(self) -> int:
        w = C.c_int(-1)
        self._check(lib().vsf_get_fast_resident(self._h, C.byref(w)), "vsf_get_fast_resident")
        return w.value

    # ---- detection masks (detectAndCompute's mask argument; include/vsf.h "Detection masks") ----
    def mask_set(self, slot: int, mask: np.ndarray):
        """BLOCKING: builds the slot's mask pyramid from a (height, width) uint8 array; non-zero = a corner may sit there."""
        mask = _u8(mask)
        self._check(lib().vsf_mask_set(self._h, int(slot), _p(mask), mask.shape[1], mask.shape[0], mask.strides[0]),
                    "vsf_mask_set")

    def mask_set_dev(self, slot: int, d_mask: int, w: int, h: int, stride: int):
        self._check(lib().vsf_mask_set_dev(self._h, int(slot), C.c_void_p(d_mask), w, h, stride), "vsf_mask_set_dev")

    def mask_clear(self, slot: int):
        self._check(lib().vsf_mask_clear(self._h, int(slot)), "vsf_mask_clear")

    def mask_is_set(self, slot: int) -> bool:
        v = C.c_int()
        self._check(lib().vsf_mask_is_set(self._h, int(slot), C.byref(v)), "vsf_mask_is_set")
        return bool(v.value)

    def mask_slot_bytes(self) -> int:
        v = C.c_size_t()
        self._check(lib().vsf_mask_slot_bytes(self._h, C.byref(v)), "vsf_mask_slot_bytes")
        return int(v.value)

    def set_image_masks(self, even_slot: int = NO_MASK, odd_slot: int = NO_MASK):
        """Image i of the extraction calls takes even_slot when i is even (the left eye), odd_slot when odd; -1: none."""
        self._check(lib().vsf_set_image_masks(self._h, int(even_slot), int(odd_slot)), "vsf_set_image_masks")

    def get_image_masks(self):
        a, b = C.c_int(), C.c_int()
        self._check(lib().vsf_get_image_masks(self._h, C.byref(a), C.byref(b)), "vsf_get_image_masks")
        return a.value, b.value

    def observe_set_stream_masks(self, stream: int, left_slot: int = NO_MASK, right_slot: int = NO_MASK):
        """The queue's frames of `stream` submitted from now on take these slots (left image, right image); -1: none."""
        self._check(lib().vsf_observe_set_stream_masks(self._h, int(stream), int(left_slot), int(right_slot)),
                    "vsf_observe_set_stream_masks")

    def debug_mask_level(self, slot: int, level: int) -> np.ndarray:
        w, h, _, _ = self.level_info(level)
        out = np.empty((h, w), np.uint8)
        self._check(lib().vsf_debug_mask_level(self._h, int(slot), level, _p(out), w), "vsf_debug_mask_level")
        return out

    def set_pipeline(self, on: bool):
        self._check(lib().vsf_set_pipeline(self._h, int(on)), "vsf_set_pipeline")

    def set_input_event(self, hip_event):
        """The next batched call (its pipelined pyramid included) waits on the GPU for this hipEvent_t (an int handle,
        e.g. torch.cuda.Event.cuda_event after record()); one-shot; None withdraws it."""
        self._check(lib().vsf_set_input_event(self._h, C.c_void_p(int(hip_event) if hip_event else None)), "vsf_set_input_event")

    def reserve(self, n_frames: int, n_pairs: int):
        """BLOCKING set-up: scratch of the batched *_dev calls for up to n_frames stereo frames / n_pairs temporal pairs."""
        self._check(lib().vsf_reserve(self._h, int(n_frames), int(n_pairs)), "vsf_reserve")

    def sync(self, allow_capacity: bool = False) -> int:
        return self._check(lib().vsf_sync(self._h), "vsf_sync", allow_capacity)

    # ---- host-pointer API (one call == one reference call) ----
    def extract(self, img: np.ndarray, cap: int | None = None):
        """detectAndCompute: returns (keypoints[KEYPOINT_DTYPE], descriptors[n,32] uint8)."""
        img = _u8(img)
        cap = self.params.max_keypoints if cap is None else cap
        kp = np.zeros(max(cap, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(cap, 1), DESC_BYTES), np.uint8)
        n = C.c_int()
        self._check(lib().vsf_extract(self._h, _p(img), img.shape[1], img.shape[0], img.strides[0], _p(kp), _p(desc),
                                      cap, C.byref(n)), "vsf_extract")
        return kp[:n.value], desc[:n.value]

    def extract_pair(self, img0: np.ndarray, img1: np.ndarray, cap: int | None = None):
        """Both detectAndCompute calls of a stereo frame in one batch: ((kp0, desc0), (kp1, desc1))."""
        img0, img1 = _u8(img0), _u8(img1)
        assert img0.shape == img1.shape and img0.strides == img1.strides
        cap = self.params.max_keypoints if cap is None else cap
        kp = [np.zeros(max(cap, 1), KEYPOINT_DTYPE) for _ in range(2)]
        desc = [np.zeros((max(cap, 1), DESC_BYTES), np.uint8) for _ in range(2)]
        n0, n1 = C.c_int(), C.c_int()
        self._check(lib().vsf_extract_pair(self._h, _p(img0), _p(img1), img0.shape[1], img0.shape[0], img0.strides[0],
                                           _p(kp[0]), _p(desc[0]), C.byref(n0), _p(kp[1]), _p(desc[1]), C.byref(n1), cap),
                    "vsf_extract_pair")
        return (kp[0][:n0.value], desc[0][:n0.value]), (kp[1][:n1.value], desc[1][:n1.value])

    def get_matches_multi(self, q_sets, t: np.ndarray):
        """GetMatches of every query set against one train set in one call: list of DMATCH arrays."""
        q_sets = [_desc(q) for q in q_sets]
        t = _desc(t)
        S = len(q_sets)
        cap = max(max((len(q) for q in q_sets), default=0), 1)
        ptrs = (C.c_void_p * S)(*[q.ctypes.data if len(q) else None for q in q_sets])
        nq = np.array([len(q) for q in q_sets], np.int32)
        out = np.zeros((S, cap), DMATCH_DTYPE)
        n_out = np.zeros(S, np.int32)
        self._check(lib().vsf_get_matches_multi(self._h, C.cast(ptrs, C.c_void_p), _p(nq), S, _p(t), len(t), _p(out), cap,
                                                _p(n_out)), "vsf_get_matches_multi")
        return [out[s, :n_out[s]].copy() for s in range(S)]

    def fast_detect(self, img: np.ndarray, threshold: int = -1, nms: bool = True, cap: int = 1 << 16):
        img = _u8(img)
        kp = np.zeros(max(cap, 1), KEYPOINT_DTYPE)
        n = C.c_int()
        self._check(lib().vsf_fast_detect(self._h, _p(img), img.shape[1], img.shape[0], img.strides[0], threshold,
                                          int(nms), _p(kp), cap, C.byref(n)), "vsf_fast_detect")
        return kp[:n.value]

    def knn2_hamming(self, q: np.ndarray, t: np.ndarray):
        q, t = _desc(q), _desc(t)
        idx = np.full((max(len(q), 1), 2), -1, np.int32)
        dist = np.full((max(len(q), 1), 2), np.iinfo(np.int32).max, np.int32)
        self._check(lib().vsf_knn2_hamming(self._h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)),
                    "vsf_knn2_hamming")
        return idx[:len(q)], dist[:len(q)]

    def get_matches(self, q: np.ndarray, t: np.ndarray) -> np.ndarray:
        q, t = _desc(q), _desc(t)
        out = np.zeros(max(len(q), 1), DMATCH_DTYPE)
        n = C.c_int()
        self._check(lib().vsf_get_matches(self._h, _p(q), len(q), _p(t), len(t), _p(out), len(q), C.byref(n)),
                    "vsf_get_matches")
        return out[:n.value]

    # ---- device-pointer API (raw addresses, e.g. tensor.data_ptr()) ----
    def extract_batch_dev(self, d_imgs: int, n_images: int, image_stride: int, row_stride: int, d_kp: int,
                          d_desc: int, d_counts: int):
        self._check(lib().vsf_extract_batch_dev(self._h, _p(d_imgs), n_images, image_stride, row_stride, _p(d_kp),
                                                _p(d_desc), _p(d_counts)), "vsf_extract_batch_dev")

    def match_batch_dev(self, d_desc: int, d_counts: int, set_stride: int, d_q_set: int, d_t_set: int, n_pairs: int,
                        d_idx2: int, d_dist2: int, d_matches: int, d_nmatches: int):
        self._check(lib().vsf_match_batch_dev(self._h, _p(d_desc), _p(d_counts), set_stride, _p(d_q_set),
                                              _p(d_t_set), n_pairs, _p(d_idx2), _p(d_dist2), _p(d_matches),
                                              _p(d_nmatches)), "vsf_match_batch_dev")

    def stereo_batch_dev(self, d_imgs: int, n_frames: int, image_stride: int, row_stride: int, d_kp: int,
                         d_desc: int, d_counts: int, d_matches: int, d_nmatches: int):
        self._check(lib().vsf_stereo_batch_dev(self._h, _p(d_imgs), n_frames, image_stride, row_stride, _p(d_kp),
                                               _p(d_desc), _p(d_counts), _p(d_matches), _p(d_nmatches)),
                    "vsf_stereo_batch_dev")

    def remove_ambig_stereo_batch_dev(self, d_kp: int, d_desc: int, d_matches: int, d_nmatches: int, n_frames: int,
                                      F: np.ndarray, thr_in: float, d_thr_override: int, d_means: int, d_thr: int,
                                      d_kp_out: int, d_desc_out: int, d_counts_out: int):
        Fh = np.ascontiguousarray(F, np.float32).reshape(9)
        self._check(lib().vsf_remove_ambig_stereo_batch_dev(self._h, _p(d_kp), _p(d_desc), _p(d_matches), _p(d_nmatches),
                                                            n_frames, _p(Fh), thr_in, _p(d_thr_override), _p(d_means),
                                                            _p(d_thr), _p(d_kp_out), _p(d_desc_out), _p(d_counts_out)),
                    "vsf_remove_ambig_stereo_batch_dev")

    def feature_matches_batch_dev(self, d_desc: int, d_counts: int, set_stride: int, d_q_set: int, d_t_set: int,
                                  n_pairs: int, best_percent: float, d_pairs: int, d_npairs: int):
        self._check(lib().vsf_feature_matches_batch_dev(self._h, _p(d_desc), _p(d_counts), set_stride, _p(d_q_set),
                                                        _p(d_t_set), n_pairs, best_percent, _p(d_pairs), _p(d_npairs)),
                    "vsf_feature_matches_batch_dev")

    def stereo_residuals_batch_dev(self, d_kp: int, d_matches: int, d_nmatches: int, n_frames: int, F: np.ndarray,
                                   d_means: int):
        Fh = np.ascontiguousarray(F, np.float32).reshape(9)
        self._check(lib().vsf_stereo_residuals_batch_dev(self._h, _p(d_kp), _p(d_matches), _p(d_nmatches), n_frames,
                                                         _p(Fh), _p(d_means)), "vsf_stereo_residuals_batch_dev")

    def stereo_thresholds_dev(self, d_means: int, n: int, d_thr_state: int, d_thr: int):
        self._check(lib().vsf_stereo_thresholds_dev(self._h, _p(d_means), n, _p(d_thr_state), _p(d_thr)),
                    "vsf_stereo_thresholds_dev")

    def stereo_filter_batch_dev(self, d_kp: int, d_desc: int, d_matches: int, d_nmatches: int, n_frames: int,
                                d_thr: int, d_kp_out: int, d_desc_out: int, d_counts_out: int):
        self._check(lib().vsf_stereo_filter_batch_dev(self._h, _p(d_kp), _p(d_desc), _p(d_matches), _p(d_nmatches),
                                                      n_frames, _p(d_thr), _p(d_kp_out), _p(d_desc_out),
                                                      _p(d_counts_out)), "vsf_stereo_filter_batch_dev")

    def vision_features_batch_dev(self, calib: VsfCalibration, d_kp: int, d_desc: int, d_counts: int, n_frames: int,
                                  d_features: int, d_nfeatures: int, d_npoints: int = 0):
        self._check(lib().vsf_vision_features_batch_dev(self._h, C.byref(calib), _p(d_kp), _p(d_desc), _p(d_counts),
                                                        n_frames, _p(d_features), _p(d_nfeatures), _p(d_npoints)),
                    "vsf_vision_features_batch_dev")

    def world_points_batch_dev(self, d_features: int, d_nfeatures: int, n_frames: int, poses, cam_to_robot, d_points: int,
                               d_npoints: int):
        """AddFeaturePoints of n_frames frames on the device (vsf_world_points_batch_dev).  poses: (n_frames, 7) float32
        rows of loc xyz + quaternion xyzw (vsf_pose); cam_to_robot: 3 x 4 float32, row-major."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(n_frames, 7)
        c = np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)
        self._check(lib().vsf_world_points_batch_dev(self._h, _p(d_features), _p(d_nfeatures), n_frames, _p(poses), _p(c),
                                                     _p(d_points), _p(d_npoints)), "vsf_world_points_batch_dev")

    def world_points(self, features: np.ndarray, pose, cam_to_robot) -> np.ndarray:
        """The same for one frame's VISION_FEATURE_DTYPE records in host memory (vsf_world_points): the (n, 3) float64 points."""
        f = np.ascontiguousarray(features, VISION_FEATURE_DTYPE)
        pose = np.ascontiguousarray(pose, np.float32).reshape(7)
        c = np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)
        out = np.zeros((max(len(f), 1), 3), np.float64)
        n = C.c_int(0)
        self._check(lib().vsf_world_points(self._h, _p(f), len(f), _p(pose), _p(c), _p(out), len(f), C.byref(n)), "vsf_world_points")
        return out[:n.value].copy()

    def observe_set_world_points(self, on: bool, cam_to_robot=None, allow_status=()) -> int:
        """The queue's point cloud (vsf_observe_set_world_points); cam_to_robot: 3 x 4 float32, row-major.  Returns the status."""
        c = None if cam_to_robot is None else np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)
        st = lib().vsf_observe_set_world_points(self._h, int(bool(on)), _p(c) if c is not None else None)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_world_points", lib().vsf_last_hip_error(self._h))
        return st

    def observe_set_pose(self, stream: int, loc, quat_xyzw):
        """The pose the frames submitted afterwards on `stream` carry (vsf_observe_set_pose)."""
        l = np.ascontiguousarray(loc, np.float32).reshape(3)
        q = np.ascontiguousarray(quat_xyzw, np.float32).reshape(4)
        self._check(lib().vsf_observe_set_pose(self._h, stream, _p(l), _p(q)), "vsf_observe_set_pose")

    def observe_set_debug_seeds(self, seeds, allow_status=()) -> int:
        """A colour generator per stream (vsf_observe_set_debug_seeds): one seed per stream, None: the process's rand() again.
        Returns the status."""
        v = None if seeds is None else np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        st = lib().vsf_observe_set_debug_seeds(self._h, _p(v) if v is not None else None, 0 if v is None else len(v))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_debug_seeds", lib().vsf_last_hip_error(self._h))
        return st

    def observe_set_stream_cam_to_robot(self, stream: int, cam_to_robot=None, allow_status=()) -> int:
        """A stream's own left_cam_to_robot, 3 x 4 float32 (vsf_observe_set_stream_cam_to_robot); None: the context's again."""
        c = None if cam_to_robot is None else np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)
        st = lib().vsf_observe_set_stream_cam_to_robot(self._h, stream, _p(c) if c is not None else None)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_stream_cam_to_robot", lib().vsf_last_hip_error(self._h))
        return st

    def observe_world_points(self, ticket: int, allow_status=()):
        """A collected frame's points (vsf_observe_world_points_view), copied: an (n, 3) float64 array -- or, with
        `allow_status`, (status, array)."""
        ptr, n = C.c_void_p(), C.c_int32(0)
        st = lib().vsf_observe_world_points_view(self._h, C.c_int64(ticket), C.byref(ptr), C.byref(n))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_world_points_view", lib().vsf_last_hip_error(self._h))
        pts = np.zeros((0, 3), np.float64)
        if st == VSF_OK and n.value > 0:
            pts = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n.value, 3)).copy()
        return (st, pts) if allow_status else pts

    def packed_outputs_capacity(self, n_frames: int, n_pairs: int) -> int:
        return int(lib().vsf_packed_outputs_capacity(self._h, n_frames, n_pairs))

    def pack_outputs_dev(self, d_features: int, d_nfeatures: int, n_frames: int, d_pairs: int, d_npairs: int,
                         n_pairs: int, d_payload: int, payload_cap: int):
        self._check(lib().vsf_pack_outputs_dev(self._h, _p(d_features), _p(d_nfeatures), n_frames, _p(d_pairs),
                                               _p(d_npairs), n_pairs, _p(d_payload), payload_cap),
                    "vsf_pack_outputs_dev")

    def observe_stereo(self, left: np.ndarray, right: np.ndarray, calib: VsfCalibration, best_percent: float = 0.3,
                       frame_life: int = 10) -> dict:
        """One Frontend::ObserveImage worth of GPU work in one submission (vsf_observe_stereo); returns the decoded
        result: header fields, `features` (VISION_FEATURE_DTYPE), `factors` (FEATURE_MATCH_DTYPE arrays, oldest kept
        frame first), `stereo_pairs` (the right->left matches of Calculate3DPoints), `keypoints`, `descriptors`."""
        left, right = _u8(left), _u8(right)
        assert left.shape == right.shape and left.strides == right.strides
        cap = int(lib().vsf_observe_capacity(self._h, frame_life))
        buf = np.zeros(max(cap, 64), np.uint8)
        n = C.c_size_t()
        self._check(lib().vsf_observe_stereo(self._h, _p(left), _p(right), left.shape[1], left.shape[0], left.strides[0],
                                             C.byref(calib), float(np.float32(best_percent)), frame_life, _p(buf), cap,
                                             C.byref(n)), "vsf_observe_stereo")
        return decode_observation(buf[:n.value])

    def observe_submit(self, left: np.ndarray, right: np.ndarray, calib: VsfCalibration, best_percent: float = 0.3,
                       frame_life: int = 10) -> int:
        """Queues one ObserveImage (vsf_observe_submit) and returns its ticket without waiting for the GPU."""
        left, right = _u8(left), _u8(right)
        assert left.shape == right.shape and left.strides == right.strides
        t = C.c_int64(-1)
        self._check(lib().vsf_observe_submit(self._h, _p(left), _p(right), left.shape[1], left.shape[0], left.strides[0],
                                             C.byref(calib), float(np.float32(best_percent)), frame_life, C.byref(t)),
                    "vsf_observe_submit")
        return int(t.value)

    def observe_set_streams(self, n_streams: int, allow_status=()) -> int:
        """The queue takes frames of `n_streams` independent sequences (vsf_observe_set_streams); returns the status."""
        st = lib().vsf_observe_set_streams(self._h, n_streams)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_streams", lib().vsf_last_hip_error(self._h))
        if st == VSF_OK and n_streams != self._n_streams:  # (another count drops the declared input sizes)
            self._input_sizes = {}
            self._n_streams = n_streams
        return st

    def observe_reset_stream(self, stream: int):
        """Forgets one stream's window and threshold (vsf_observe_reset_stream)."""
        self._check(lib().vsf_observe_reset_stream(self._h, stream), "vsf_observe_reset_stream")

    def observe_set_input_size(self, stream: int, width: int, height: int, allow_status=()) -> int:
        """The size the frames of `stream` arrive at (vsf_observe_set_input_size): the queue brings them to the context's size
        with cv::resize on the device.  (0, 0): the context's size again.  Returns the status."""
        st = lib().vsf_observe_set_input_size(self._h, stream, width, height)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_input_size", lib().vsf_last_hip_error(self._h))
        if st == VSF_OK:
            self._input_sizes[stream] = (width, height) if width or height else None
        return st

    def observe_submit_stream(self, stream: int, left: np.ndarray, right: np.ndarray, calib: VsfCalibration,
                              best_percent: float = 0.3, frame_life: int = 10, allow_status=()):
        """vsf_observe_submit_stream: queues one ObserveImage of sequence `stream`.  Returns the ticket -- or, with
        `allow_status`, (status, ticket): a refused submit has ticket -1."""
        left, right = _u8(left), _u8(right)
        assert left.shape == right.shape and left.strides == right.strides
        t = C.c_int64(-1)
        st = lib().vsf_observe_submit_stream(self._h, stream, _p(left), _p(right), left.shape[1], left.shape[0],
                                             left.strides[0], C.byref(calib), float(np.float32(best_percent)), frame_life,
                                             C.byref(t))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_stream", lib().vsf_last_hip_error(self._h))
        return (st, int(t.value)) if allow_status else int(t.value)

    def observe_submit_stream_pix(self, stream: int, left: np.ndarray, right: np.ndarray, pixfmt: int, calib: VsfCalibration,
                                  best_percent: float = 0.3, frame_life: int = 10, allow_status=(), width: int = None,
                                  stride: int = None):
        """vsf_observe_submit_stream_pix: one raw host frame of any PIX_* format -- (h, w) arrays for MONO8 and the Bayer
        orders, (h, w, 3 or 4) for packed colour.  width / stride override what the arrays say (for refusal tests).  Returns
        the ticket -- or, with `allow_status`, (status, ticket)."""
        left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
        if left.strides[-1] != 1 or (left.ndim == 3 and left.strides[1] != left.shape[2]):
            left = np.ascontiguousarray(left)
        if right.strides != left.strides or right.shape != left.shape:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
        assert left.shape == right.shape and left.strides == right.strides and left.ndim in (2, 3)
        t = C.c_int64(-1)
        st = lib().vsf_observe_submit_stream_pix(self._h, stream, _p(left), _p(right), left.shape[1] if width is None else width,
                                                 left.shape[0], left.strides[0] if stride is None else stride, pixfmt,
                                                 C.byref(calib), float(np.float32(best_percent)), frame_life, C.byref(t))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_stream_pix", lib().vsf_last_hip_error(self._h))
        return (st, int(t.value)) if allow_status else int(t.value)

    def observe_set_bayer_order(self, stream: int, pixfmt: int, allow_status=()) -> int:
        """vsf_observe_set_bayer_order: the order of the mosaics `stream`'s compressed submits carry with bayer=True."""
        st = lib().vsf_observe_set_bayer_order(self._h, stream, pixfmt)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_set_bayer_order", lib().vsf_last_hip_error(self._h))
        return st

    def observe_submit_compressed_stream(self, stream: int, left: bytes, right: bytes, calib: VsfCalibration,
                                         bayer: bool = False, best_percent: float = 0.3, frame_life: int = 10,
                                         allow_status=()):
        """vsf_observe_submit_compressed_stream; returns (status, ticket) like observe_submit_compressed."""
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        t = C.c_int64(-1)
        st = lib().vsf_observe_submit_compressed_stream(self._h, stream, _p(lb), len(lb), _p(rb), len(rb), int(bool(bayer)),
                                                        C.byref(calib), float(np.float32(best_percent)), frame_life,
                                                        C.byref(t))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_compressed_stream", lib().vsf_last_hip_error(self._h))
        return st, int(t.value)

    def observe_submit_dev(self, frames, calib: VsfCalibration, stream: int = 0, pixfmt: int = PIX_MONO8,
                           producer_stream: int | None = None, best_percent: float = 0.3, frame_life: int = 10,
                           allow_status=()):
        """vsf_observe_submit_dev: queues len(frames) consecutive frames of sequence `stream` that already live in device
        memory, stream-ordered on `producer_stream` (a hipStream_t as an integer; None: torch.cuda.current_stream() of the
        context's device).  A frame is a pair (left, right) of 2-D torch.uint8 tensors on the context's device (device_image:
        ValueError otherwise, before the library is called), or four integers (left address, left pitch, right address,
        right pitch).  Returns the tickets -- or, with `allow_status`, (status, tickets): a refused call's are all -1."""
        p = self.params
        w, h = self._input_sizes.get(stream) or (p.width, p.height)  # (observe_set_input_size)
        arr = (VsfDevFrame * max(len(frames), 1))()
        for i, f in enumerate(frames):
            if len(f) == 2:
                (lp, ls), (rp, rs) = (device_image_pix(t, w, h, self.device, pixfmt) for t in f)
            else:
                lp, ls, rp, rs = (int(v) for v in f)
            arr[i] = VsfDevFrame(lp, rp, ls, rs)
        if producer_stream is None:
            import torch
            producer_stream = torch.cuda.current_stream(self.device).cuda_stream
        tickets = (C.c_int64 * max(len(frames), 1))(*([-1] * max(len(frames), 1)))
        st = lib().vsf_observe_submit_dev(self._h, stream, arr, len(frames), pixfmt, C.c_void_p(producer_stream or None),
                                          C.byref(calib), float(np.float32(best_percent)), frame_life, tickets)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_dev", lib().vsf_last_hip_error(self._h))
        out = [int(t) for t in tickets[:len(frames)]]
        return (st, out) if allow_status else out

    def observe_device_ring_bytes(self, depth: int = 0) -> int:
        """HBM the queue's device ring takes at `depth` (vsf_observe_device_ring_bytes; no device work)."""
        return int(lib().vsf_observe_device_ring_bytes(self._h, depth))

    def observe_collect(self, ticket: int, frame_life: int = 10) -> dict:
        """Waits for the frame of `ticket` (vsf_observe_collect) and returns its decoded result."""
        cap = int(lib().vsf_observe_capacity(self._h, frame_life))
        buf = np.zeros(max(cap, 64), np.uint8)
        n = C.c_size_t()
        self._check(lib().vsf_observe_collect(self._h, C.c_int64(ticket), _p(buf), cap, C.byref(n)), "vsf_observe_collect")
        return decode_observation(buf[:n.value])

    def observe_submit_compressed(self, left: bytes, right: bytes, calib: VsfCalibration, bayer: bool = False,
                                  best_percent: float = 0.3, frame_life: int = 10, allow_status=()):
        """Queues one ObserveImage given as two CompressedImage payloads (vsf_observe_submit_compressed: JPEG or PNG, decoded
        on the GPU inside the batch).  Returns (status, ticket); a status not in `allow_status` raises, and a refused submit
        has ticket -1."""
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        t = C.c_int64(-1)
        st = lib().vsf_observe_submit_compressed(self._h, _p(lb), len(lb), _p(rb), len(rb), int(bool(bayer)), C.byref(calib),
                                                 float(np.float32(best_percent)), frame_life, C.byref(t))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_compressed", lib().vsf_last_hip_error(self._h))
        return st, int(t.value)

    def observe_stereo_compressed(self, left: bytes, right: bytes, calib: VsfCalibration, bayer: bool = False,
                                  best_percent: float = 0.3, frame_life: int = 10) -> dict:
        """vsf_observe_stereo_compressed: submit + collect of one frame given as two compressed payloads."""
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        cap = int(lib().vsf_observe_capacity(self._h, frame_life))
        buf = np.zeros(max(cap, 64), np.uint8)
        n = C.c_size_t()
        self._check(lib().vsf_observe_stereo_compressed(self._h, _p(lb), len(lb), _p(rb), len(rb), int(bool(bayer)),
                                                        C.byref(calib), float(np.float32(best_percent)), frame_life,
                                                        _p(buf), cap, C.byref(n)), "vsf_observe_stereo_compressed")
        return decode_observation(buf[:n.value])

    def observe_submit_compressed_reduced(self, left: bytes, right: bytes, calib: VsfCalibration, reduce: int, stream: int = 0,
                                          best_percent: float = 0.3, frame_life: int = 10, allow_status=()):
        """vsf_observe_submit_compressed_reduced: one ObserveImage given as two JPEG payloads read as
        cv::imdecode(IMREAD_REDUCED_GRAYSCALE_<reduce>) reads them (files of up to `reduce` times the context's size a side;
        the calibration is the caller's, for the reduced image).  Returns (status, ticket) like observe_submit_compressed."""
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        t = C.c_int64(-1)
        st = lib().vsf_observe_submit_compressed_reduced(self._h, stream, _p(lb), len(lb), _p(rb), len(rb), reduce, C.byref(calib),
                                                         float(np.float32(best_percent)), frame_life, C.byref(t))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_submit_compressed_reduced", lib().vsf_last_hip_error(self._h))
        return st, int(t.value)

    def observe_stereo_compressed_reduced(self, left: bytes, right: bytes, calib: VsfCalibration, reduce: int,
                                          best_percent: float = 0.3, frame_life: int = 10) -> dict:
        """vsf_observe_stereo_compressed_reduced: submit + collect of one such frame."""
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        cap = int(lib().vsf_observe_capacity(self._h, frame_life))
        buf = np.zeros(max(cap, 64), np.uint8)
        n = C.c_size_t()
        self._check(lib().vsf_observe_stereo_compressed_reduced(self._h, _p(lb), len(lb), _p(rb), len(rb), reduce, C.byref(calib),
                                                                float(np.float32(best_percent)), frame_life, _p(buf), cap,
                                                                C.byref(n)), "vsf_observe_stereo_compressed_reduced")
        return decode_observation(buf[:n.value])

    def observe_collect_bytes(self, ticket: int, frame_life: int = 10, allow_status=()):
        """vsf_observe_collect as (status, the result's bytes): what the tests compare byte for byte.  Header word 13
        (bytes 52..56) is the decoder status of a compressed frame (include/vsf.h)."""
        cap = int(lib().vsf_observe_capacity(self._h, frame_life))
        buf = np.zeros(max(cap, 64), np.uint8)
        n = C.c_size_t()
        st = lib().vsf_observe_collect(self._h, C.c_int64(ticket), _p(buf), cap, C.byref(n))
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_observe_collect", lib().vsf_last_hip_error(self._h))
        return st, buf[:n.value].copy()

    def observe_set_compressed_cap(self, cap_per_image: int):
        """Bytes a compressed payload may have (vsf_observe_set_compressed_cap; 0: width x height + 64 KB)."""
        self._check(lib().vsf_observe_set_compressed_cap(self._h, cap_per_image), "vsf_observe_set_compressed_cap")

    def observe_stats(self) -> dict:
        """vsf_observe_stats by name."""
        v = np.zeros(len(OBSERVE_STATS), np.int64)
        self._check(lib().vsf_observe_stats(self._h, _p(v), len(v)), "vsf_observe_stats")
        return {k: int(x) for k, x in zip(OBSERVE_STATS, v)}

    def debug_jpeg_serial(self, on: bool):
        """Test hook: every JPEG file through the one-wave-per-image decoder (vsf_debug_jpeg_serial)."""
        lib().vsf_debug_jpeg_serial.argtypes = [C.c_void_p, C.c_int]
        self._check(lib().vsf_debug_jpeg_serial(self._h, int(on)), "vsf_debug_jpeg_serial")

    def observe_reset(self):
        self._check(lib().vsf_observe_reset(self._h), "vsf_observe_reset")

    def observe_poll(self, ticket: int) -> bool:
        """True when the frame's result is there (vsf_observe_poll: does not wait, sends nothing)."""
        r = C.c_int(0)
        self._check(lib().vsf_observe_poll(self._h, C.c_int64(ticket), C.byref(r)), "vsf_observe_poll")
        return bool(r.value)

    def observe_configure(self, depth: int = 0, min_batch: int = 0, in_flight: int = 0):
        """The ObserveImage queue (vsf_observe_configure): frames that may wait uncollected, the fewest waiting frames that
        leave while the GPU is busy, batches on the GPU at a time (0 = the defaults)."""
        self._check(lib().vsf_observe_configure(self._h, depth, min_batch, in_flight), "vsf_observe_configure")

    def jpeg_decode_gray_batch(self, files, width: int, height: int, d_dst: int, dst_image_stride: int,
                               dst_row_stride: int, allow_status=()):
        """cv::imdecode(IMREAD_GRAYSCALE) of baseline-JPEG files (bytes objects, host) into device memory
        (slam_frontend_main.cc:99-100); asynchronous on the context's stream.  Returns the status (VSF_OK unless listed
        in `allow_status`)."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        st = lib().vsf_jpeg_decode_gray_batch(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, width,
                                              height, _p(d_dst), dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_jpeg_decode_gray_batch", lib().vsf_last_hip_error(self._h))
        return st

    def png_decode_gray_batch(self, files, width: int, height: int, d_dst: int, dst_image_stride: int,
                              dst_row_stride: int, allow_status=()):
        """cv::imdecode(IMREAD_GRAYSCALE) of grayscale PNG files (bytes objects, host) into device memory
        (slam_frontend_main.cc:99-100); asynchronous on the context's stream."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        st = lib().vsf_png_decode_gray_batch(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, width,
                                             height, _p(d_dst), dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_png_decode_gray_batch", lib().vsf_last_hip_error(self._h))
        return st

    def draw_canvases_dev(self, canvases, d_ops: int, n_ops: int):
        """vsf_draw_canvases_dev: canvases is a list of dicts with the fields of VsfDrawCanvas (device pointers as ints);
        d_ops points at n_ops DRAW_OP_DTYPE records in device memory.  Asynchronous on the context's stream."""
        arr = (VsfDrawCanvas * max(len(canvases), 1))()
        for i, c in enumerate(canvases):
            for k, v in c.items():
                setattr(arr[i], k, v)
        return self._check(lib().vsf_draw_canvases_dev(self._h, arr, len(canvases), C.c_void_p(d_ops or None), n_ops),
                           "vsf_draw_canvases_dev")

    def imdecode_gray_batch(self, files, width: int, height: int, d_dst: int, dst_image_stride: int,
                            dst_row_stride: int, allow_status=()):
        """cv::imdecode(IMREAD_GRAYSCALE) of JPEG and PNG payloads, mixed (slam_frontend_main.cc:99-100)."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        st = lib().vsf_imdecode_gray_batch(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, width, height,
                                           _p(d_dst), dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_imdecode_gray_batch", lib().vsf_last_hip_error(self._h))
        return st

    def imdecode_bgr_batch(self, files, width: int, height: int, d_dst: int, dst_image_stride: int, dst_row_stride: int,
                           allow_status=(), only: str = ""):
        """cv::imdecode(IMREAD_COLOR) of JPEG and PNG payloads, mixed (vsf_imdecode_bgr_batch): image i at
        d_dst + i * dst_image_stride, rows of 3 * width bytes (blue, green, red) dst_row_stride apart.  only = "jpeg" / "png":
        the call of that one format (vsf_jpeg_decode_bgr_batch / vsf_png_decode_bgr_batch)."""
        name = {"": "vsf_imdecode_bgr_batch", "jpeg": "vsf_jpeg_decode_bgr_batch", "png": "vsf_png_decode_bgr_batch"}[only]
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        st = getattr(lib(), name)(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, width, height,
                                  _p(d_dst), dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, name, lib().vsf_last_hip_error(self._h))
        return st

    def imdecode_reduced_gray_batch(self, files, reduce: int, width: int, height: int, d_dst: int, dst_image_stride: int,
                                    dst_row_stride: int, allow_status=()):
        """cv::imdecode(IMREAD_REDUCED_GRAYSCALE_<reduce>) of JPEG payloads (vsf_imdecode_reduced_gray_batch): width x height
        is the OUTPUT size, ceil(W / reduce) x ceil(H / reduce) of every file; reduce = 1 is imdecode_gray_batch."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        st = lib().vsf_imdecode_reduced_gray_batch(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, reduce, width,
                                                   height, _p(d_dst), dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_imdecode_reduced_gray_batch", lib().vsf_last_hip_error(self._h))
        return st

    def _encode_batch_dev(self, fmt: str, quality: tuple, d_src, n_images, width, height, channels, src_image_stride, src_row_stride,
                          d_out, out_stride, d_out_bytes):
        """vsf_<fmt>_encode_batch_dev; `quality`: the arguments between the strides and d_out ((quality,) for JPEG, () for PNG)."""
        name = "vsf_%s_encode_batch_dev" % fmt
        self._check(getattr(lib(), name)(self._h, _p(d_src), n_images, width, height, channels, src_image_stride, src_row_stride,
                                         *quality, _p(d_out), out_stride, _p(d_out_bytes)), name)

    def _encode(self, fmt: str, quality: tuple, images, out_stride):
        """vsf_<fmt>_encode of equally sized (h, w) gray or (h, w, 3) BGR uint8 images -> list of bytes."""
        imgs = np.ascontiguousarray(np.stack([np.asarray(i) for i in images]), dtype=np.uint8)
        n, h, w = imgs.shape[:3]
        ch = 1 if imgs.ndim == 3 else imgs.shape[3]
        name = "vsf_%s_encode" % fmt
        stride = int(getattr(lib(), name + "_capacity")(w, h, ch)) if out_stride is None else out_stride
        out = np.zeros((n, stride), np.uint8)
        nbytes = np.zeros(n, np.int32)
        self._check(getattr(lib(), name)(self._h, _p(imgs), n, w, h, ch, w * h * ch, w * ch, *quality, _p(out), stride, _p(nbytes)),
                    name)
        return [out[i, :nbytes[i]].tobytes() for i in range(n)]

    def jpeg_encode_batch_dev(self, d_src: int, n_images: int, width: int, height: int, channels: int, src_image_stride: int,
                              src_row_stride: int, quality: int, d_out: int, out_stride: int, d_out_bytes: int):
        """cv::imencode(".jpg") of images resident in HBM: file i at d_out + i * out_stride, its size in d_out_bytes[i]."""
        self._encode_batch_dev("jpeg", (quality,), d_src, n_images, width, height, channels, src_image_stride, src_row_stride, d_out,
                               out_stride, d_out_bytes)

    def jpeg_encode(self, images, quality: int = 0, out_stride: int | None = None):
        """cv::imencode(".jpg", img, quality) of equally sized (h, w) gray or (h, w, 3) BGR uint8 images -> list of bytes."""
        return self._encode("jpeg", (quality,), images, out_stride)

    def png_encode_batch_dev(self, d_src: int, n_images: int, width: int, height: int, channels: int, src_image_stride: int,
                             src_row_stride: int, d_out: int, out_stride: int, d_out_bytes: int):
        """cv::imencode(".png") of images resident in HBM: file i at d_out + i * out_stride, its size in d_out_bytes[i]."""
        self._encode_batch_dev("png", (), d_src, n_images, width, height, channels, src_image_stride, src_row_stride, d_out, out_stride,
                               d_out_bytes)

    def png_encode(self, images, out_stride: int | None = None):
        """cv::imencode(".png", img) of equally sized (h, w) gray or (h, w, 3) BGR uint8 images -> list of bytes."""
        return self._encode("png", (), images, out_stride)

    def resize_gray_batch_dev(self, d_src: int, n_images: int, src_width: int, src_height: int, src_image_stride: int,
                              src_row_stride: int, d_dst: int, dst_width: int, dst_height: int, dst_image_stride: int,
                              dst_row_stride: int, allow_status=()) -> int:
        """cv::resize (INTER_LINEAR, CV_8UC1) of images resident in HBM (vsf_resize_gray_batch_dev): any sizes in 1 .. 32767,
        any base address, any pitch >= the width.  Asynchronous on the context's stream.  Returns the status."""
        st = lib().vsf_resize_gray_batch_dev(self._h, _p(d_src), n_images, src_width, src_height, src_image_stride,
                                             src_row_stride, _p(d_dst), dst_width, dst_height, dst_image_stride, dst_row_stride)
        if st != VSF_OK and st not in allow_status:
            raise VsfError(st, "vsf_resize_gray_batch_dev", lib().vsf_last_hip_error(self._h))
        return st

    def resize_gray(self, images, dst_width: int, dst_height: int) -> np.ndarray:
        """cv::resize (INTER_LINEAR, CV_8UC1) of equally sized (h, w) uint8 images in host memory (vsf_resize_gray): an
        (n, dst_height, dst_width) array."""
        imgs = np.ascontiguousarray(np.stack([np.asarray(i) for i in images]), dtype=np.uint8)
        n, h, w = imgs.shape
        out = np.zeros((n, dst_height, dst_width), np.uint8)
        self._check(lib().vsf_resize_gray(self._h, _p(imgs), n, w, h, w * h, w, _p(out), dst_width, dst_height,
                                          dst_width * dst_height, dst_width), "vsf_resize_gray")
        return out

    def bayer_bg_to_gray_batch_dev(self, d_src: int, n_images: int, width: int, height: int, src_image_stride: int,
                                   src_row_stride: int, d_dst: int, dst_image_stride: int, dst_row_stride: int):
        """DecodeImage's BayerBG2BGR + BGR2GRAY (slam_frontend_main.cc:101-106) on mosaics resident in HBM."""
        self._check(lib().vsf_bayer_bg_to_gray_batch_dev(self._h, _p(d_src), n_images, width, height, src_image_stride,
                                                         src_row_stride, _p(d_dst), dst_image_stride, dst_row_stride),
                    "vsf_bayer_bg_to_gray_batch_dev")

    def to_gray(self, imgs: np.ndarray, pixfmt: int) -> np.ndarray:
        """vsf_to_gray: (n, h, w) or (n, h, w, 3 or 4) raw images in host memory -> (n, h, w) gray images."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        n, h, w = imgs.shape[:3]
        row = w * (imgs.shape[3] if imgs.ndim == 4 else 1)
        out = np.zeros((n, h, w), np.uint8)
        self._check(lib().vsf_to_gray(self._h, _p(imgs), n, w, h, pixfmt, row * h, row, _p(out), w * h, w), "vsf_to_gray")
        return out

    def to_gray_batch_dev(self, d_src: int, n_images: int, width: int, height: int, pixfmt: int, src_image_stride: int,
                          src_row_stride: int, d_dst: int, dst_image_stride: int, dst_row_stride: int) -> int:
        """vsf_to_gray_batch_dev: raw images of any PIX_* format resident in HBM -> gray, one launch.  Returns the status."""
        return lib().vsf_to_gray_batch_dev(self._h, _p(d_src), n_images, width, height, pixfmt, src_image_stride,
                                           src_row_stride, _p(d_dst), dst_image_stride, dst_row_stride)

    def to_bgr(self, imgs: np.ndarray, pixfmt: int) -> np.ndarray:
        """vsf_to_bgr: (n, h, w) or (n, h, w, 3 or 4) raw images in host memory -> (n, h, w, 3) B G R images."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        n, h, w = imgs.shape[:3]
        row = w * (imgs.shape[3] if imgs.ndim == 4 else 1)
        out = np.zeros((n, h, w, 3), np.uint8)
        self._check(lib().vsf_to_bgr(self._h, _p(imgs), n, w, h, pixfmt, row * h, row, _p(out), 3 * w * h, 3 * w), "vsf_to_bgr")
        return out

    def to_bgr_batch_dev(self, d_src: int, n_images: int, width: int, height: int, pixfmt: int, src_image_stride: int,
                         src_row_stride: int, d_dst: int, dst_image_stride: int, dst_row_stride: int) -> int:
        """vsf_to_bgr_batch_dev: raw images of any PIX_* format resident in HBM -> B G R (vsf_imdecode_bgr_batch's layout), one
        launch.  Returns the status."""
        return lib().vsf_to_bgr_batch_dev(self._h, _p(d_src), n_images, width, height, pixfmt, src_image_stride,
                                          src_row_stride, _p(d_dst), dst_image_stride, dst_row_stride)

    def bag_extract_batch(self, files, width: int, height: int, bayer_pixfmt: int = 0, quality: int = 0,
                          out_stride: int | None = None, allow_status=()):
        """src/test/bag_extract.cc:73-90 for JPEG / PNG payloads of one size (vsf_bag_extract_batch): colour read, on a Bayer
        topic (bayer_pixfmt = one of the four PIX_BAYER_* codes) channel 0 demosaiced in that order, colour JPEG files.
        Returns (status, files): files[i] is bytes, or None where out_bytes[i] is -1."""
        n = len(files)
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
        stride = int(lib().vsf_jpeg_encode_capacity(width, height, 3)) if out_stride is None else out_stride
        out = np.zeros((max(n, 1), max(stride, 1)), np.uint8)
        nbytes = np.zeros(max(n, 1), np.int32)
        st = lib().vsf_bag_extract_batch(self._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, width, height,
                                         bayer_pixfmt, quality, _p(out), stride, _p(nbytes))
        if st not in (VSF_OK, VSF_ERR_CAPACITY) and st not in allow_status:
            raise VsfError(st, "vsf_bag_extract_batch", lib().vsf_last_hip_error(self._h))
        return st, [out[i, :nbytes[i]].tobytes() if nbytes[i] >= 0 else None for i in range(n)]

    def debug_retain_best(self, keys: np.ndarray, n_points: int, use_lds: bool = False, mode: int = 0):
        """retainBest on the GPU; returns (keys, ids) of the survivors in the order the GPU left them."""
        kb = np.ascontiguousarray(keys).view(np.uint32).copy()
        ids = np.arange(len(kb), dtype=np.uint32)
        n = C.c_int()
        self._check(lib().vsf_debug_retain_best(self._h, _p(kb), _p(ids), len(kb), n_points, int(use_lds), mode,
                                                C.byref(n)), "vsf_debug_retain_best")
        return kb[:n.value], ids[:n.value]

    def debug_retain_best_form(self, form: str, stage: int, keys: np.ndarray, n_points: int, level_cap: int | None = None,
                               poison: tuple = (0xAB, 0xCDEF01)):
        """retainBest as ONE stage of the production selection kernel runs it.  form: "A" wide, "B" common, "C" 9 216-entry,
        "D" tiny (SELECT_FORMS); stage 1: keys are score bytes 0..255, stage 2: float32 responses.  level_cap (default
        len(keys) + 19) is the capacity of the level's scratch slices; the entries behind the array hold `poison`.
        Returns (keys, ids, tail_intact): survivors as uint32 key bits (stage 1: the byte) and ids in the device's order,
        and whether everything behind the array came back untouched."""
        n = len(keys)
        cap = n + 19 if level_cap is None else level_cap
        kb = np.full(cap, poison[0], np.uint32)
        ids = np.full(cap, poison[1], np.uint32)
        kb[:n] = np.asarray(keys).astype(np.uint32) if stage == 1 else np.ascontiguousarray(keys, np.float32).view(np.uint32)
        ids[:n] = np.arange(n, dtype=np.uint32)
        m = C.c_int()
        self._check(lib().vsf_debug_retain_best_form(self._h, "ABCD".index(form), stage, _p(kb), _p(ids), n, n_points, cap,
                                                     C.byref(m)), "vsf_debug_retain_best_form")
        intact = bool((kb[n:] == poison[0]).all() and (ids[n:] == poison[1]).all())
        return kb[:m.value], ids[:m.value], intact

    def debug_sort_trim(self, matches: np.ndarray, best_percent: float = 1.0, serial: bool = False):
        """matches: (n_lists, n) DMATCH_DTYPE.  Returns a list of (queryIdx, trainIdx) int arrays, one per list: the first
        int(n * best_percent) matches in the order the device's restatement of std::sort leaves them."""
        m = np.ascontiguousarray(matches, DMATCH_DTYPE)
        if m.ndim == 1:
            m = m[None]
        nl, n = m.shape
        pairs = np.zeros((nl, max(n, 1), 2), np.uint64)
        counts = np.zeros(nl, np.int32)
        self._check(lib().vsf_debug_sort_trim(self._h, _p(m), nl, n, float(np.float32(best_percent)), int(serial),
                                              _p(pairs), _p(counts)), "vsf_debug_sort_trim")
        return [pairs[i, :counts[i]].astype(np.int64) for i in range(nl)]

    # ---- per-stage device timing ----
    def profile_enable(self, on: bool = True):
        self._check(lib().vsf_profile_enable(self._h, int(on)), "vsf_profile_enable")

    def profile_read(self, reset: bool = True) -> dict:
        """{stage name: (total ms, launches)} since the last reset (synchronises the stream)."""
        ms = (C.c_double * STAGE_COUNT)()
        n = (C.c_int64 * STAGE_COUNT)()
        self._check(lib().vsf_profile_read(self._h, ms, n, int(reset)), "vsf_profile_read")
        return {lib().vsf_stage_name(i).decode(): (ms[i], int(n[i])) for i in range(STAGE_COUNT)}

    # ---- introspection ----
    def debug_level_image(self, image: int, level: int, blurred: bool = False) -> np.ndarray:
        w, h, _, _ = self.level_info(level)
        out = np.empty((h, w), np.uint8)
        self._check(lib().vsf_debug_level_image(self._h, image, level, int(blurred), _p(out), w),
                    "vsf_debug_level_image")
        return out

    def debug_fast_candidates(self, image: int, level: int, cap: int = 1 << 17) -> np.ndarray:
        kp = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._check(lib().vsf_debug_fast_candidates(self._h, image, level, _p(kp), cap, C.byref(n)),
                    "vsf_debug_fast_candidates")
        return kp[:min(n.value, cap)]

    def debug_describe_form(self, n_images: int) -> int:
        """Keypoints per wave (4 or 8) of the describe kernel one launch over n_images images takes (vsf_debug_describe_form)."""
        form = lib().vsf_debug_describe_form(self._h, int(n_images))
        if form not in (4, 8):
            raise VsfError(form, "vsf_debug_describe_form")
        return form

    def debug_level_keypoints(self, image: int, level: int, cap: int = 1 << 15) -> np.ndarray:
        kp = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._check(lib().vsf_debug_level_keypoints(self._h, image, level, _p(kp), cap, C.byref(n)),
                    "vsf_debug_level_keypoints")
        return kp[:min(n.value, cap)]


def _u8(img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    if img.strides[1] != 1:
        img = np.ascontiguousarray(img)
    return img


def _desc(d: np.ndarray) -> np.ndarray:
    d = np.ascontiguousarray(d, np.uint8)
    return d.reshape(-1, DESC_BYTES)


def unpack_outputs(payload: np.ndarray):
    """Inverse of vsf_pack_outputs_dev: (list of VISION_FEATURE_DTYPE arrays per frame, list of FEATURE_MATCH_DTYPE
    arrays per pair).  `payload`: uint8 array holding at least the packed bytes."""
    b = np.ascontiguousarray(payload, np.uint8).reshape(-1)
    hdr = b[:16].view(np.uint32)
    if int(hdr[0]) != PAYLOAD_MAGIC:
        raise ValueError("not a packed output payload")
    nf, npairs, total = int(hdr[1]), int(hdr[2]), int(hdr[3])
    if total > len(b):
        raise ValueError("payload truncated: %d of %d bytes" % (len(b), total))
    counts = b[16:16 + 4 * (nf + npairs)].view(np.uint32).astype(np.int64)
    off = 16 + 4 * (nf + npairs)
    feats, matches = [], []
    for i in range(nf):
        n = int(counts[i]) * 28
        feats.append(b[off:off + n].view(VISION_FEATURE_DTYPE).copy())
        off += n
    for i in range(npairs):
        n = int(counts[nf + i]) * 16
        matches.append(b[off:off + n].view(FEATURE_MATCH_DTYPE).copy())
        off += n
    assert off == total
    return feats, matches


def decode_observation(buf: np.ndarray) -> dict:
    """Decodes vsf_observe_stereo's result (layout: include/vsf.h)."""
    b = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    hdr = b[:64].view(np.uint32)
    if int(hdr[0]) != 0x4F465356:
        raise ValueError("not an observation payload")
    n_pairs, nfeat, total = int(hdr[1]), int(hdr[2]), int(hdr[3])
    assert total == len(b), (total, len(b))
    f32 = b[:64].view(np.float32)
    npairs = b[64:64 + 4 * n_pairs].view(np.uint32).astype(np.int64)
    off = 64 + 4 * ((n_pairs + 3) & ~3)
    feats = b[off:off + 28 * nfeat].view(VISION_FEATURE_DTYPE).copy()
    off += 28 * nfeat
    lists = []
    for p in range(n_pairs):
        lists.append(b[off:off + 16 * int(npairs[p])].view(FEATURE_MATCH_DTYPE).copy())
        off += 16 * int(npairs[p])
    kp = b[off:off + 28 * nfeat].view(KEYPOINT_DTYPE).copy()
    off += 28 * nfeat
    desc = b[off:off + 32 * nfeat].reshape(nfeat, 32).copy()
    off += 32 * nfeat
    assert off == total
    return {"n_left": int(hdr[4]), "n_right": int(hdr[5]), "n_stereo_matches": int(hdr[6]), "n_points": int(hdr[7]),
            "mean": np.float32(f32[8]), "threshold": np.float32(f32[9]), "threshold_next": np.float32(f32[10]),
            "decoder_status": int(hdr[13]), "features": feats, "factors": lists[:-1], "stereo_pairs": lists[-1], "keypoints": kp, "descriptors": desc}
