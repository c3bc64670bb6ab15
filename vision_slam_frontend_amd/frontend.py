"""ctypes view of the C++ host class slam::Frontend (vision_slam_frontend_amd/host/, libvsf_frontend.so), the
mirror of the reference's Frontend::ObserveImage / ObserveOdometry / GetSLAMProblem API on top of the HIP C ABI.
Used by tests and examples; the class itself is C++ because the reference's is."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import capi

LIB_PATH = Path(__file__).resolve().parent / "libvsf_frontend.so"
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        capi.lib()  # libvsf_hip.so first (fails loudly if it was not built)
        if not LIB_PATH.exists():
            raise ImportError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        L = C.CDLL(str(LIB_PATH))
        vp, i32, f32, sz, dbl = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_double
        L.vsfh_frontend_create.argtypes = [i32, i32, i32, i32, vp, f32, i32]
        L.vsfh_frontend_create.restype = vp
        L.vsfh_frontend_create_score.argtypes = [i32, i32, i32, i32, vp, f32, i32, i32]
        L.vsfh_frontend_create_score.restype = vp
        L.vsfh_frontend_destroy.argtypes = [vp]
        L.vsfh_observe_odometry.argtypes = [vp, vp, vp, dbl]
        L.vsfh_observe_image.argtypes = [vp, vp, vp, i32, i32, sz, dbl]
        L.vsfh_observe_compressed_image.argtypes = [vp, vp, sz, vp, sz, i32, dbl]
        L.vsfh_observe_device_image.argtypes = [vp, vp, sz, vp, sz, vp, dbl, i32]
        L.vsfh_observe_image_pix.argtypes = [vp, vp, vp, i32, i32, sz, i32, dbl]
        L.vsfh_observe_device_image_pix.argtypes = [vp, vp, sz, vp, sz, vp, dbl, i32]
        L.vsfh_group_observe_image_pix.argtypes = [vp, i32, vp, vp, i32, i32, sz, i32, dbl]
        L.vsfh_group_observe_device_image_pix.argtypes = [vp, i32, vp, sz, vp, sz, vp, dbl, i32]
        L.vsfh_set_bayer_order.argtypes = [vp, i32]
        L.vsfh_set_bayer_order.restype = None
        L.vsfh_group_observe_device_image.argtypes = [vp, i32, vp, sz, vp, sz, vp, dbl, i32]
        L.vsfh_last_status.argtypes = [vp]
        L.vsfh_refused_frames.argtypes = [vp]
        L.vsfh_refused_frames.restype = C.c_uint64
        L.vsfh_num_poses.argtypes = [vp]
        L.vsfh_stereo_ambig_constraint.argtypes = [vp]
        L.vsfh_stereo_ambig_constraint.restype = f32
        L.vsfh_get_fundamental.argtypes = [vp, vp]
        L.vsfh_num_vision_factors.argtypes = [vp]
        L.vsfh_vision_factor.argtypes = [vp, i32, vp, vp, vp, i32]
        L.vsfh_node.argtypes = [vp, i32, vp, vp, vp, vp, i32]
        L.vsfh_num_odometry_factors.argtypes = [vp]
        L.vsfh_odometry_factor.argtypes = [vp, i32, vp, vp]
        L.vsfh_frame.argtypes = [vp, i32, vp, vp, vp, i32]
        L.vsfh_serialize_problem.argtypes = [vp, vp, sz]
        L.vsfh_serialize_problem.restype = sz
        L.vsfh_default_calibration.argtypes = [C.POINTER(capi.VsfCalibration)]
        L.vsfh_default_calibration.restype = None
        L.vsfh_set_fused.argtypes = [vp, i32]
        L.vsfh_set_fused.restype = None
        L.vsfh_set_pipelined.argtypes = [vp, i32]
        L.vsfh_set_pipelined.restype = None
        L.vsfh_set_frames_in_flight.argtypes = [vp, i32]
        L.vsfh_set_frames_in_flight.restype = None
        L.vsfh_set_queue.argtypes = [vp, i32, i32, i32]
        L.vsfh_set_queue.restype = None
        L.vsfh_set_queue_threads.argtypes = [vp, i32, i32]
        L.vsfh_set_queue_threads.restype = None
        L.vsfh_time_sequence.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(dbl), C.POINTER(dbl)]
        L.vsfh_time_sequence.restype = dbl
        L.vsfh_left_cam_to_robot.argtypes = [vp, vp, vp]
        L.vsfh_left_cam_to_robot.restype = None
        L.vsfh_serialize_calibration.argtypes = [vp, vp, vp]
        L.vsfh_serialize_calibration.restype = None
        L.vsfh_flush.argtypes = [vp]
        L.vsfh_set_debug_images.argtypes = [vp, i32]
        L.vsfh_set_debug_images.restype = None
        L.vsfh_num_debug_images.argtypes = [vp, i32]
        L.vsfh_debug_image.argtypes = [vp, i32, i32, vp, sz, vp]
        L.vsfh_set_debug_jpeg_quality.argtypes = [vp, i32]
        L.vsfh_set_debug_jpeg_quality.restype = None
        L.vsfh_set_debug_png.argtypes = [vp, i32]
        L.vsfh_set_debug_png.restype = None
        L.vsfh_set_debug_colour_seed.argtypes = [vp, i32, C.c_uint32]
        L.vsfh_set_debug_colour_seed.restype = None
        L.vsfh_set_left_cam_to_robot.argtypes = [vp, vp]
        L.vsfh_set_left_cam_to_robot.restype = None
        L.vsfh_group_create_ex.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, i32]
        L.vsfh_group_create_ex.restype = vp
        L.vsfh_group_create_score.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32]
        L.vsfh_group_create_score.restype = vp
        L.vsfh_set_imdecode_reduce.argtypes = [vp, i32]
        L.vsfh_set_imdecode_reduce.restype = None
        L.vsfh_set_resize.argtypes = [vp, i32, i32, i32, i32]
        L.vsfh_set_resize.restype = None
        L.vsfh_set_masks.argtypes = [vp, vp, vp, i32, i32, sz]
        L.vsfh_set_masks.restype = None
        L.vsfh_set_compressed_cap.argtypes = [vp, sz]
        L.vsfh_set_compressed_cap.restype = None
        L.vsfh_debug_image_compressed_format.argtypes = [vp, i32]
        L.vsfh_debug_image_compressed.argtypes = [vp, i32, vp, sz]
        L.vsfh_debug_image_compressed.restype = sz
        L.vsfh_group_create.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32]
        L.vsfh_group_create.restype = vp
        L.vsfh_group_destroy.argtypes = [vp]
        L.vsfh_group_destroy.restype = None
        L.vsfh_group_size.argtypes = [vp]
        L.vsfh_group_member.argtypes = [vp, i32]
        L.vsfh_group_member.restype = vp
        L.vsfh_group_last_status.argtypes = [vp]
        L.vsfh_group_set_pipelined.argtypes = [vp, i32]
        L.vsfh_group_set_pipelined.restype = None
        L.vsfh_group_set_queue.argtypes = [vp, i32, i32, i32]
        L.vsfh_group_set_queue.restype = None
        L.vsfh_group_set_queue_thread.argtypes = [vp, i32]
        L.vsfh_group_set_queue_thread.restype = None
        L.vsfh_group_flush.argtypes = [vp]
        L.vsfh_group_observe_odometry.argtypes = [vp, i32, vp, vp, dbl]
        L.vsfh_group_observe_odometry.restype = None
        L.vsfh_group_observe_image.argtypes = [vp, i32, vp, vp, i32, i32, sz, dbl]
        L.vsfh_group_observe_compressed_image.argtypes = [vp, i32, vp, sz, vp, sz, i32, dbl]
        L.vsfh_group_queue_stats.argtypes = [vp, vp, i32]
        L.vsfh_group_serialize_problem.argtypes = [vp, i32, vp, sz]
        L.vsfh_group_serialize_problem.restype = sz
        L.vsfh_set_projections.argtypes = [vp, vp, vp]
        L.vsfh_set_projections.restype = None
        L.vsfh_set_visualization.argtypes = [vp, i32]
        L.vsfh_set_visualization.restype = None
        L.vsfh_group_set_visualization.argtypes = [vp, i32]
        L.vsfh_group_set_visualization.restype = None
        L.vsfh_visualization_points.argtypes = [vp, i32, i32, vp, sz]
        L.vsfh_visualization_points.restype = C.c_longlong
        L.vsfh_serialize_visualization.argtypes = [vp, i32, i32, vp, sz]
        L.vsfh_serialize_visualization.restype = sz
        L.vsfh_add_feature_points.argtypes = [vp, vp, vp, vp, i32, vp]
        L.vsfh_time_visualization.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_longlong)]
        L.vsfh_time_visualization.restype = dbl
        L.vsfh_queue_stats.argtypes = [vp, vp, i32]
        L.vsfh_bag_extract_create.argtypes = [i32, i32, i32]
        L.vsfh_bag_extract_create.restype = vp
        L.vsfh_bag_extract_destroy.argtypes = [vp]
        L.vsfh_bag_extract_destroy.restype = None
        L.vsfh_bag_extract_run.argtypes = [vp, vp, vp, i32, C.c_char_p, vp, sz, C.POINTER(i32), C.POINTER(i32)]
        L.vsfh_bag_extract_run.restype = sz
        L.vsfh_bag_extract_path.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, vp, sz]
        L.vsfh_bag_extract_path.restype = sz
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _host_frame(left, right, pixfmt: int):
    """Two raw host images of one PIX_* format -- (h, w), or (h, w, 3 or 4) for packed colour -- as contiguous arrays, with
    their width in pixels and their row stride in bytes."""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    bpp = capi.pixfmt_bytes_per_pixel(pixfmt)
    assert left.shape == right.shape and (left.ndim == 2 if bpp <= 1 else left.ndim == 3 and left.shape[2] == bpp), left.shape
    return left, right, left.shape[1], left.shape[0], left.strides[0]


def _device_frame(left, right, width: int, height: int, device: int, stream, pixfmt: int = 0):
    """What vsfh_observe_device_image takes of two tensors: (left address, left pitch, right address, right pitch, stream).
    ValueError -- before any call into the library -- for a tensor that is not height x width torch.uint8 with dense rows on
    GPU `device`; stream None: torch.cuda.current_stream() of that device, else a torch stream or a hipStream_t as an integer."""
    (lp, ls), (rp, rs) = (capi.device_image_pix(t, width, height, device, pixfmt) for t in (left, right))
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    return lp, ls, rp, rs, C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)


def add_feature_points(cam_to_robot, loc, quat_xyzw, point3d) -> np.ndarray:
    """The CPU restatement of the point cloud (host/slam_visualization.h AddFeaturePoints, the reference's
    slam_frontend_main.cc:155-173) on ONE node with the given pose and features: the kept points, (n, 3) float64.  No GPU."""
    c = np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)
    l = np.ascontiguousarray(loc, np.float32).reshape(3)
    q = np.ascontiguousarray(quat_xyzw, np.float32).reshape(4)
    p = np.ascontiguousarray(point3d, np.float32).reshape(-1, 3)
    out = np.zeros((max(len(p), 1), 3), np.float64)
    n = lib().vsfh_add_feature_points(_p(c), _p(l), _p(q), _p(p), len(p), _p(out))
    return out[:n].copy()


def bag_extract_path(output: str, count: int, index: int) -> str:
    """slam::BagExtractPath: the reference's file name for message `index` of `count` (src/test/bag_extract.cc:81-87)."""
    buf = C.create_string_buffer(len(output) + 64)
    n = lib().vsfh_bag_extract_path(output.encode(), count, index, buf, len(buf))
    return buf.raw[:n].decode()


class BagExtract:
    """slam::BagExtract (host/bag_extract.h): serialized sensor_msgs/CompressedImage messages -> colour JPEG files on disk, as
    src/test/bag_extract.cc writes them; decode, demosaic and encode run on the GPU (vsf_bag_extract_batch)."""

    def __init__(self, device: int = 0, quality: int = 0, max_per_call: int = 512):
        self._h = lib().vsfh_bag_extract_create(device, quality, max_per_call)
        self.last_status = capi.VSF_OK
        self.calls = 0

    def close(self):
        if self._h:
            lib().vsfh_bag_extract_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, messages, output: str):
        """-> the paths written, in message order ('' where a message gave no file; see last_status)."""
        blob = np.frombuffer(b"".join(bytes(m) for m in messages) or b"\0", np.uint8)
        offsets = np.zeros(len(messages) + 1, np.uint64)
        offsets[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        st, calls = C.c_int32(0), C.c_int32(0)
        buf = C.create_string_buffer((len(output) + 64) * max(len(messages), 1))
        n = lib().vsfh_bag_extract_run(self._h, _p(blob), _p(offsets), len(messages), output.encode(), buf, len(buf),
                                       C.byref(st), C.byref(calls))
        assert n <= len(buf)
        self.last_status, self.calls = st.value, calls.value
        return buf.raw[:n].decode().split("\n")[:len(messages)]


def default_calibration() -> capi.VsfCalibration:
    """FrontendConfig()'s stereo calibration (the reference's hard-coded constants, slam_frontend.cc:565-644)."""
    c = capi.VsfCalibration()
    lib().vsfh_default_calibration(C.byref(c))
    return c


class Frontend:
    def __init__(self, width: int, height: int, nfeatures: int = 10000, device: int = 0, fundamental=None,
                 best_percent: float = 0.0, frame_life: int = 0, debug_images: bool = False,
                 debug_jpeg_quality: int = 0, debug_png: bool = False, visualization: bool = False, imdecode_reduce: int = 1,
                 compressed_cap: int = 0, debug_colour_seed=None, cam_to_robot=None, resize_to=None,
                 score_type: int = capi.HARRIS_SCORE, masks=None):
        """score_type: FrontendConfig::orb_score_type_ (capi.HARRIS_SCORE, the reference's, or capi.FAST_SCORE).
        masks=(left, right): FrontendConfig::mask_left_ / mask_right_ -- detectAndCompute's mask argument per eye, uint8 arrays
        of the context's size (the resized size with resize_to), non-zero where a corner may sit; None for an eye: no mask.
        resize_to=(w, h): FrontendConfig::resize_width_ / resize_height_ -- the context has that size, width x height is
        the CAMERA's (what device frames are taken to be; raw and compressed frames bring their own), every frame goes through
        cv::resize on the device, and the calibration is the caller's, for the resized image."""
        F = None if fundamental is None else np.ascontiguousarray(fundamental, np.float32).reshape(9)
        cw, ch = (width, height) if resize_to is None else (int(resize_to[0]), int(resize_to[1]))
        self._h = lib().vsfh_frontend_create_score(nfeatures, cw, ch, device, _p(F), best_percent, frame_life, int(score_type))
        self.cap = nfeatures + 256
        self.size, self.device = (width, height), device
        if resize_to is not None:
            lib().vsfh_set_resize(self._h, cw, ch, width, height)
        if masks is not None:
            self.set_masks(*masks)
        if debug_colour_seed is not None:  # FrontendConfig::debug_colour_seeded_ / _seed_: the object's own rand(), before the switch
            lib().vsfh_set_debug_colour_seed(self._h, 1, int(debug_colour_seed))
        if debug_images:  # FrontendConfig::debug_images_ (the reference's default is on, slam_frontend.cc:552)
            lib().vsfh_set_debug_images(self._h, 1)
        if debug_jpeg_quality:  # FrontendConfig::debug_jpeg_quality_: the queued modes keep JPEG files instead of raw images
            lib().vsfh_set_debug_jpeg_quality(self._h, debug_jpeg_quality)
        if debug_png:  # FrontendConfig::debug_png_: ... or PNG files, lossless (not together with the JPEG form)
            lib().vsfh_set_debug_png(self._h, 1)
        if cam_to_robot is not None:  # FrontendConfig::left_cam_to_robot, 3 x 4 row-major
            lib().vsfh_set_left_cam_to_robot(self._h, _p(np.ascontiguousarray(cam_to_robot, np.float32).reshape(12)))
        if visualization:  # FrontendConfig::visualization_: the point cloud and pose graph of Frontend::GetVisualization
            lib().vsfh_set_visualization(self._h, 1)
        if imdecode_reduce != 1:  # FrontendConfig::imdecode_reduce_: IMREAD_REDUCED_GRAYSCALE_N; width x height is the reduced size
            lib().vsfh_set_imdecode_reduce(self._h, int(imdecode_reduce))
        if compressed_cap:  # FrontendConfig::compressed_cap_: bytes a payload may have (the default is sized by width x height)
            lib().vsfh_set_compressed_cap(self._h, int(compressed_cap))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend")

    def set_masks(self, left=None, right=None):
        """FrontendConfig::mask_left_ / mask_right_ (Frontend::set_masks): the object keeps copies; None: no mask for that eye."""
        arrs = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in (left, right)]
        shapes = {a.shape for a in arrs if a is not None}
        if len(shapes) > 1 or any(len(s) != 2 for s in shapes):
            raise ValueError("masks are 2-D uint8 arrays of one size")
        h, w = shapes.pop() if shapes else (0, 0)
        lib().vsfh_set_masks(self._h, _p(arrs[0]), _p(arrs[1]), w, h, w)
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend.set_masks")

    def set_fused(self, on: bool):
        """True (default): ObserveImage is one GPU submission (vsf_observe_stereo); False: one C-ABI call per
        reference call with the reference's host steps in between.  Choose before the first observe_image."""
        lib().vsfh_set_fused(self._h, int(on))

    def set_pipelined(self, on: bool):
        """observe_image queues its frame on the GPU and returns (its return value is the odometry gate's decision); results
        are collected and booked, in frame order, two frames later or when the problem is read.  Fused mode; choose before the
        first observe_image."""
        lib().vsfh_set_pipelined(self._h, int(on))

    def set_frames_in_flight(self, n: int):
        """How many frames a pipelined Frontend leaves in the context's queue (1..1024; default 256).  Choose before the first
        observe_image."""
        lib().vsfh_set_frames_in_flight(self._h, int(n))

    def set_queue(self, depth: int = 0, batch_frames: int = 0, min_batch: int = 0):
        """The ObserveImage queue of a pipelined Frontend: frames that may wait uncollected (default 256), frames per batch at
        most (default 128: sizes the context), fewest waiting frames that leave while the GPU is busy (0: a whole batch, or half the depth when that is less).
        Choose before the first observe_image."""
        lib().vsfh_set_queue(self._h, int(depth), int(batch_frames), int(min_batch))

    def set_queue_threads(self, launcher: bool = False, copy: bool = True):
        """The queue's host threads (VSF_OPT_OBSERVE_THREAD / VSF_OPT_OBSERVE_COPY_THREAD).  Choose before the first
        observe_image."""
        lib().vsfh_set_queue_threads(self._h, int(launcher), int(copy))

    def time_sequence(self, frames: np.ndarray, n_frames: int, warm: int = 32, read_every: int = 0):
        """The reference's driver loop in C++ (vsfh_time_sequence) over `frames` [n][2][h][w] taken in turn: returns
        (steady frames per second, mean ms inside ObserveImage, max ms)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 4 and frames.shape[1] == 2
        mean, worst = C.c_double(), C.c_double()
        fps = lib().vsfh_time_sequence(self._h, _p(frames), frames.shape[0], frames.shape[3], frames.shape[2], int(n_frames),
                                       int(warm), int(read_every), C.byref(mean), C.byref(worst))
        if fps < 0:
            raise capi.VsfError(lib().vsfh_last_status(self._h), "Frontend::ObserveImage (time_sequence)")
        return float(fps), float(mean.value), float(worst.value)

    def _debug_image(self, stereo: bool, i: int):
        shape = np.zeros(3, np.int32)
        if not lib().vsfh_debug_image(self._h, int(stereo), i, None, 0, _p(shape)):
            return None
        out = np.zeros(tuple(int(v) for v in shape), np.uint8)
        lib().vsfh_debug_image(self._h, int(stereo), i, _p(out), out.nbytes, _p(shape))
        return out

    def debug_images(self, stereo: bool = False):
        """getDebugImages() (stereo: getDebugStereoImages()) as rows x cols x 3 arrays, bytes in OpenCV's B, G, R order."""
        return [self._debug_image(stereo, i) for i in range(lib().vsfh_num_debug_images(self._h, int(stereo)))]

    def last_debug_image_compressed(self, stereo: bool = False):
        """GetLastDebugImageCompressed() (stereo: GetLastDebugStereoImageCompressed()) as bytes; None when there is none."""
        n = lib().vsfh_debug_image_compressed(self._h, int(stereo), None, 0)
        if not n:
            return None
        out = np.zeros(n, np.uint8)
        lib().vsfh_debug_image_compressed(self._h, int(stereo), _p(out), n)
        return out.tobytes()

    def last_debug_image_format(self, stereo: bool = False):
        """CompressedView::format of the same getters: "jpeg", "png" or None."""
        return (None, "jpeg", "png")[lib().vsfh_debug_image_compressed_format(self._h, int(stereo))]

    def last_debug_image(self, stereo: bool = False):
        """GetLastDebugImage() (stereo: GetLastDebugStereoImage()); None for the reference's empty cv::Mat."""
        return self._debug_image(stereo, -1)

    def flush(self) -> bool:
        """Collects and books every frame still in flight."""
        return bool(lib().vsfh_flush(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().vsfh_frontend_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def observe_odometry(self, translation, rotation_wxyz, timestamp: float):
        t = np.ascontiguousarray(translation, np.float32)
        q = np.ascontiguousarray(rotation_wxyz, np.float32)
        lib().vsfh_observe_odometry(self._h, _p(t), _p(q), timestamp)

    def set_bayer_order(self, pixfmt: int):
        """FrontendConfig::bayer_order_: the order of the mosaics observe_compressed_image(bayer_rggb8=True) decodes (one of
        capi.PIX_BAYER_*).  Legal at any time; VsfError(INVALID_ARG) and no change for anything else."""
        lib().vsfh_set_bayer_order(self._h, int(pixfmt))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::set_bayer_order")

    def observe_image(self, left: np.ndarray, right: np.ndarray, time: float = 0.0, pixfmt: int = capi.PIX_MONO8) -> bool:
        """Frontend::ObserveImage.  pixfmt: what the arrays hold (capi.PIX_*): (h, w) for mono8 and the Bayer orders,
        (h, w, 3 or 4) for packed colour -- sensor_msgs/Image as the driver publishes it, made gray on the GPU."""
        if pixfmt != capi.PIX_MONO8:
            left, right, w, h, stride = _host_frame(left, right, pixfmt)
            added = bool(lib().vsfh_observe_image_pix(self._h, _p(left), _p(right), w, h, stride, pixfmt, time))
            st = lib().vsfh_last_status(self._h)
            if st != capi.VSF_OK:
                raise capi.VsfError(st, "Frontend::ObserveImage")
            return added
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        assert left.shape == right.shape and left.ndim == 2
        added = bool(lib().vsfh_observe_image(self._h, _p(left), _p(right), left.shape[1], left.shape[0],
                                              left.strides[0], time))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::ObserveImage")
        return added

    def observe_device_image(self, left, right, time: float = 0.0, bayer_rggb8: bool = False, stream=None,
                             pixfmt: int | None = None) -> bool:
        """Frontend::ObserveDeviceImage: the frame as two 2-D torch.uint8 tensors that already live on the Frontend's GPU
        (stride(1) == 1, any stride(0)), stream-ordered on `stream` (None: torch.cuda.current_stream()): they may still be
        being written by work queued on that stream, and may be overwritten by work queued on it afterwards.  A tensor of
        another dtype, device, size or inner stride raises ValueError before the library is called."""
        if pixfmt is not None:  # (any capi.PIX_* format; packed colour: (h, w, 3 or 4) tensors with dense pixels)
            lp, ls, rp, rs, s = _device_frame(left, right, self.size[0], self.size[1], self.device, stream, pixfmt)
            added = bool(lib().vsfh_observe_device_image_pix(self._h, lp, ls, rp, rs, s, time, int(pixfmt)))
            st = lib().vsfh_last_status(self._h)
            if st != capi.VSF_OK:
                raise capi.VsfError(st, "Frontend::ObserveDeviceImage")
            return added
        lp, ls, rp, rs, s = _device_frame(left, right, self.size[0], self.size[1], self.device, stream)
        added = bool(lib().vsfh_observe_device_image(self._h, lp, ls, rp, rs, s, time, int(bool(bayer_rggb8))))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::ObserveDeviceImage")
        return added

    def set_imdecode_reduce(self, reduce: int):
        """FrontendConfig::imdecode_reduce_: 1 (IMREAD_GRAYSCALE) or 2, 4, 8 (IMREAD_REDUCED_GRAYSCALE_N) for the compressed
        frames observed from now on.  The calibration is the caller's, for the reduced image."""
        lib().vsfh_set_imdecode_reduce(self._h, int(reduce))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::set_imdecode_reduce")

    def set_compressed_cap(self, cap_per_image: int):
        """FrontendConfig::compressed_cap_: bytes one compressed payload may have (0: width x height + 64 KB of the object's
        image size -- the REDUCED size with imdecode_reduce > 1, so files of a larger camera usually need this).  Before the
        first compressed frame or while no frame is in flight; a group member sets the group's."""
        lib().vsfh_set_compressed_cap(self._h, int(cap_per_image))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::set_compressed_cap")

    def observe_compressed_image(self, left: bytes, right: bytes, bayer_rggb8: bool = False, time: float = 0.0,
                                 allow_status=(), reduce: int | None = None) -> bool:
        """Frontend::ObserveCompressedImage: the two CompressedImage payloads (JPEG or PNG) as they came; decoded on the GPU
        inside the queue.  A status in `allow_status` (a refused file) is left for last_status instead of raising.
        reduce: sets FrontendConfig::imdecode_reduce_ first (None: as it is)."""
        if reduce is not None:
            self.set_imdecode_reduce(reduce)
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        added = bool(lib().vsfh_observe_compressed_image(self._h, _p(lb), len(lb), _p(rb), len(rb), int(bool(bayer_rggb8)),
                                                         time))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK and st not in allow_status:
            raise capi.VsfError(st, "Frontend::ObserveCompressedImage")
        return added

    @property
    def refused_frames(self) -> int:
        """Frames booked so far whose compressed file the device refused (observed as an all-zero image); never goes back."""
        return int(lib().vsfh_refused_frames(self._h))

    @property
    def last_status(self) -> int:
        return int(lib().vsfh_last_status(self._h))

    @property
    def num_poses(self) -> int:
        return lib().vsfh_num_poses(self._h)

    @property
    def stereo_ambig_constraint(self) -> float:
        return float(lib().vsfh_stereo_ambig_constraint(self._h))

    @property
    def fundamental(self) -> np.ndarray:
        F = np.zeros(9, np.float32)
        lib().vsfh_get_fundamental(self._h, _p(F))
        return F.reshape(3, 3)

    def vision_factors(self):
        out = []
        for i in range(lib().vsfh_num_vision_factors(self._h)):
            a, b = C.c_uint64(), C.c_uint64()
            pairs = np.zeros((self.cap, 2), np.uint64)
            n = lib().vsfh_vision_factor(self._h, i, C.byref(a), C.byref(b), _p(pairs), self.cap)
            out.append((a.value, b.value, pairs[:n].copy()))
        return out

    def nodes(self):
        out = []
        for i in range(self.num_poses):
            idx, ts = C.c_uint64(), C.c_double()
            pose = np.zeros(7, np.float32)
            feat = np.zeros((self.cap, 6), np.float32)
            n = lib().vsfh_node(self._h, i, C.byref(idx), C.byref(ts), _p(pose), _p(feat), self.cap)
            out.append({"node_idx": idx.value, "timestamp": ts.value, "pose": pose, "features": feat[:n].copy()})
        return out

    def odometry_factors(self):
        out = []
        for i in range(lib().vsfh_num_odometry_factors(self._h)):
            ij = np.zeros(2, np.uint64)
            tq = np.zeros(7, np.float32)
            lib().vsfh_odometry_factor(self._h, i, _p(ij), _p(tq))
            out.append((int(ij[0]), int(ij[1]), tq))
        return out

    @property
    def left_cam_to_robot(self):
        """GetConfig().left_cam_to_robot (slam_frontend.h:96): (rotation 3 x 3, translation 3)."""
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        lib().vsfh_left_cam_to_robot(self._h, _p(R), _p(t))
        return R.reshape(3, 3), t

    def serialize_calibration(self):
        """ROS-1 payloads of the CameraExtrinsics (48 B) and CameraIntrinsics (32 B) messages the reference's driver writes
        beside the problem (slam_frontend_main.cc:341-365)."""
        e, k = np.zeros(48, np.uint8), np.zeros(32, np.uint8)
        lib().vsfh_serialize_calibration(self._h, _p(e), _p(k))
        return e.tobytes(), k.tobytes()

    def set_projections(self, left, right):
        """FrontendConfig::projection_left / projection_right (3 x 4, row-major) before the first image: another stereo rig
        than the reference's hard-coded one."""
        l = np.ascontiguousarray(left, np.float32).reshape(12)
        r = np.ascontiguousarray(right, np.float32).reshape(12)
        lib().vsfh_set_projections(self._h, _p(l), _p(r))
        st = lib().vsfh_last_status(self._h)
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "Frontend::set_projections")

    def visualization(self, host: bool = False):
        """Frontend::GetVisualization: what the reference's driver publishes to RViz after every pose, for the frames booked
        so far (it does NOT flush the queue; complete after flush()).  Returns (cloud, nodes, odometry, vision): the point
        cloud as an (n, 3) float64 array, one point per node, and the two end points of every odometry / vision factor's line
        as (m, 2, 3) arrays.  host=True: the same computed on the CPU from the whole problem, as the reference's driver does
        (GetSLAMProblem + AddFeaturePoints / AddPoseGraph; that flushes).
        Every vsfh_visualization_points is a GetVisualization of its own, and a pipelined Frontend books whatever has finished
        in each of them: a batch that lands between two reads leaves nodes and odometry lines of different moments (every node
        but the first comes with one line).  Such a torn read is taken again, a few times at the most; nothing is read more
        often than before when it is whole (an extra poll is an extra chance for the queue to send a small batch)."""
        for _ in range(4):
            out = []
            for which in (3, 0, 1, 2):
                n = lib().vsfh_visualization_points(self._h, int(host), which, None, 0)
                if n < 0:
                    raise capi.VsfError(lib().vsfh_last_status(self._h), "Frontend::GetVisualization")
                a = np.zeros((max(n, 1), 3), np.float64)
                n = min(n, lib().vsfh_visualization_points(self._h, int(host), which, _p(a), len(a)))
                out.append(a[:n].copy())
            if len(out[2]) == 2 * max(len(out[1]) - 1, 0):
                break
        return out[0], out[1], out[2].reshape(-1, 2, 3), out[3].reshape(-1, 2, 3)

    def serialize_visualization(self, host: bool = False):
        """ROS-1 payloads of the two messages the driver publishes (host/slam_to_ros.h): the visualization_msgs/MarkerArray of
        slam_frontend/pose_graph and the visualization_msgs/Marker of slam_frontend/points."""
        out = []
        for which in (0, 1):
            n = lib().vsfh_serialize_visualization(self._h, int(host), which, None, 0)
            if n == 0:
                raise capi.VsfError(lib().vsfh_last_status(self._h), "Frontend::GetVisualization")
            buf = np.zeros(n, np.uint8)
            n = min(n, lib().vsfh_serialize_visualization(self._h, int(host), which, _p(buf), n))
            out.append(buf[:n].tobytes())
        return tuple(out)

    def time_visualization(self, frames: np.ndarray, n_frames: int, warm: int = 32, host: bool = False, publish_every: int = 1):
        """The driver's loop with the visualization asked for after every node (vsfh_time_visualization): (frames/s, points)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        pts = C.c_longlong(0)
        fps = lib().vsfh_time_visualization(self._h, _p(frames), frames.shape[0], frames.shape[3], frames.shape[2], int(n_frames),
                                            int(warm), int(host), int(publish_every), C.byref(pts))
        if fps < 0:
            raise capi.VsfError(lib().vsfh_last_status(self._h), "Frontend::GetVisualization (time_visualization)")
        return fps, int(pts.value)

    def queue_stats(self) -> dict:
        """vsf_observe_stats of the object's context, by name (capi.Context.observe_stats)."""
        v = np.zeros(len(capi.OBSERVE_STATS), np.int64)
        st = lib().vsfh_queue_stats(self._h, _p(v), len(v))
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "vsf_observe_stats")
        return {k: int(x) for k, x in zip(capi.OBSERVE_STATS, v)}

    def serialize_problem(self) -> bytes:
        """ROS-1 wire bytes of vision_slam_frontend/SLAMProblem for everything observed so far (host/slam_to_ros.h)."""
        n = lib().vsfh_serialize_problem(self._h, None, 0)
        buf = np.zeros(max(n, 1), np.uint8)
        lib().vsfh_serialize_problem(self._h, _p(buf), n)
        return buf[:n].tobytes()

    def frame(self, i: int):
        fid = C.c_uint64()
        kp = np.zeros(self.cap, capi.KEYPOINT_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = lib().vsfh_frame(self._h, i, C.byref(fid), _p(kp), _p(desc), self.cap)
        if n < 0:
            raise IndexError(i)
        return fid.value, kp[:n].copy(), desc[:n].copy()


class FrontendGroup:
    """slam::FrontendGroup: several Frontend objects on ONE GPU context and ONE ObserveImage queue (member i is stream i of
    vsf_observe_set_streams).  `fundamentals` and `best_percents` (optional) are per member; `members[i]` is member i as a
    Frontend (owned by the group).  Debug images (`debug_images`, `debug_jpeg_quality`, `debug_png`: every member's) need
    `debug_colour_seeds`, one per member, in a group of more than one; `cam_to_robots` (n x 3 x 4) gives every member its own
    FrontendConfig::left_cam_to_robot, `visualization` switches every member's on."""

    def __init__(self, width: int, height: int, fundamentals, nfeatures: int = 10000, device: int = 0, best_percents=None,
                 frame_life: int = 0, imdecode_reduces=None, compressed_cap: int = 0, debug_images: bool = False,
                 debug_jpeg_quality: int = 0, debug_png: bool = False, debug_colour_seeds=None, cam_to_robots=None,
                 visualization: bool = False, resize_to=None, camera_sizes=None, score_type: int = capi.HARRIS_SCORE,
                 masks=None):
        """score_type: every member's FrontendConfig::orb_score_type_ (one context, one mode).
        masks=[(left, right) or None, ...]: FrontendConfig::mask_left_ / mask_right_ per member (width x height arrays).
        resize_to=[(w, h) or None, ...]: FrontendConfig::resize_width_ / resize_height_ per member (None: off) -- a resized
        member takes frames of its camera's size and shares the group's width x height context, so (w, h) is width x height;
        camera_sizes=[(W, H) or None, ...]: what member i's DEVICE frames are taken to be (raw and compressed frames bring
        their own size)."""
        F = np.ascontiguousarray(fundamentals, np.float32).reshape(-1, 9)
        n = len(F)
        bp = None if best_percents is None else np.ascontiguousarray(best_percents, np.float32).reshape(n)
        seeds = None if debug_colour_seeds is None else np.ascontiguousarray(debug_colour_seeds, np.uint32).reshape(n)
        c2r = None if cam_to_robots is None else np.ascontiguousarray(cam_to_robots, np.float32).reshape(n, 12)
        self._h = lib().vsfh_group_create_score(n, nfeatures, width, height, device, _p(F), _p(bp), frame_life, int(debug_images),
                                                int(debug_jpeg_quality), int(debug_png), _p(seeds), _p(c2r), int(visualization),
                                                int(score_type))
        st = lib().vsfh_group_last_status(self._h)
        if st != capi.VSF_OK:
            self.close()
            raise capi.VsfError(st, "FrontendGroup")
        self.members = []
        for i in range(n):
            m = Frontend.__new__(Frontend)
            m._h = lib().vsfh_group_member(self._h, i)
            m.cap = nfeatures + 256
            m.size, m.device = (width, height), device
            m.close = lambda: None  # (the group owns its members)
            self.members.append(m)
        for i, r in enumerate(resize_to or ()):  # per camera: FrontendConfig::resize_width_ / resize_height_ of member i
            if r is not None:
                cam = (camera_sizes or [None] * n)[i] or (0, 0)
                lib().vsfh_set_resize(self.members[i]._h, int(r[0]), int(r[1]), int(cam[0]), int(cam[1]))
                self._check(i, "FrontendGroup(resize_to=)")
                if cam != (0, 0):
                    self.members[i].size = (int(cam[0]), int(cam[1]))
        for i, m in enumerate(masks or ()):  # per camera: FrontendConfig::mask_left_ / mask_right_ of member i
            if m is not None:
                self.members[i].set_masks(*m)
        for i, d in enumerate(imdecode_reduces or ()):  # per camera: FrontendConfig::imdecode_reduce_ of member i
            self.members[i].set_imdecode_reduce(d)
        if compressed_cap:  # the group's queue has ONE byte cap: size it for the largest camera's files
            self.members[0].set_compressed_cap(compressed_cap)

    def __len__(self):
        return len(self.members)

    def set_pipelined(self, on: bool):
        lib().vsfh_group_set_pipelined(self._h, int(on))

    def set_queue(self, depth: int = 0, batch_frames: int = 0, min_batch: int = 0):
        lib().vsfh_group_set_queue(self._h, int(depth), int(batch_frames), int(min_batch))

    def set_queue_thread(self, on: bool):
        lib().vsfh_group_set_queue_thread(self._h, int(on))

    def set_visualization(self, on: bool):
        """Every member's FrontendConfig::visualization_ (before the first image); members[i].visualization() reads member i's."""
        lib().vsfh_group_set_visualization(self._h, int(on))
        for i in range(len(self.members)):
            self._check(i, "FrontendGroup::set_visualization")

    def _check(self, i: int, where: str, allow_status=()):
        st = lib().vsfh_last_status(self.members[i]._h)
        if st != capi.VSF_OK and st not in allow_status:
            raise capi.VsfError(st, where)

    def observe_odometry(self, i: int, translation, rotation_wxyz, timestamp: float):
        t = np.ascontiguousarray(translation, np.float32)
        q = np.ascontiguousarray(rotation_wxyz, np.float32)
        lib().vsfh_group_observe_odometry(self._h, i, _p(t), _p(q), timestamp)

    def observe_image(self, i: int, left: np.ndarray, right: np.ndarray, time: float = 0.0, pixfmt: int = capi.PIX_MONO8) -> bool:
        if pixfmt != capi.PIX_MONO8:  # (Frontend.observe_image's pixfmt, for member i)
            left, right, w, h, stride = _host_frame(left, right, pixfmt)
            added = bool(lib().vsfh_group_observe_image_pix(self._h, i, _p(left), _p(right), w, h, stride, pixfmt, time))
            self._check(i, "FrontendGroup::ObserveImage")
            return added
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        assert left.shape == right.shape and left.ndim == 2
        added = bool(lib().vsfh_group_observe_image(self._h, i, _p(left), _p(right), left.shape[1], left.shape[0],
                                                    left.strides[0], time))
        self._check(i, "FrontendGroup::ObserveImage")
        return added

    def observe_device_image(self, i: int, left, right, time: float = 0.0, bayer_rggb8: bool = False, stream=None,
                             pixfmt: int | None = None) -> bool:
        """FrontendGroup::ObserveDeviceImage(i, ...): Frontend.observe_device_image for member i."""
        m = self.members[i]
        if pixfmt is not None:
            lp, ls, rp, rs, s = _device_frame(left, right, m.size[0], m.size[1], m.device, stream, pixfmt)
            added = bool(lib().vsfh_group_observe_device_image_pix(self._h, i, lp, ls, rp, rs, s, time, int(pixfmt)))
            self._check(i, "FrontendGroup::ObserveDeviceImage")
            return added
        lp, ls, rp, rs, s = _device_frame(left, right, m.size[0], m.size[1], m.device, stream)
        added = bool(lib().vsfh_group_observe_device_image(self._h, i, lp, ls, rp, rs, s, time, int(bool(bayer_rggb8))))
        self._check(i, "FrontendGroup::ObserveDeviceImage")
        return added

    def observe_compressed_image(self, i: int, left: bytes, right: bytes, bayer_rggb8: bool = False, time: float = 0.0,
                                 allow_status=(), reduce: int | None = None) -> bool:
        """reduce: member i's FrontendConfig::imdecode_reduce_ from this frame on (per camera; None: as it is)."""
        if reduce is not None:
            self.members[i].set_imdecode_reduce(reduce)
        lb, rb = np.frombuffer(bytes(left), np.uint8), np.frombuffer(bytes(right), np.uint8)
        added = bool(lib().vsfh_group_observe_compressed_image(self._h, i, _p(lb), len(lb), _p(rb), len(rb),
                                                               int(bool(bayer_rggb8)), time))
        self._check(i, "FrontendGroup::ObserveCompressedImage", allow_status)
        return added

    def serialize_problem(self, i: int) -> bytes:
        """FrontendGroup::GetSLAMProblem(i) as ROS-1 wire bytes (books every frame in flight first)."""
        n = lib().vsfh_group_serialize_problem(self._h, i, None, 0)
        buf = np.zeros(max(n, 1), np.uint8)
        lib().vsfh_group_serialize_problem(self._h, i, _p(buf), n)
        return buf[:n].tobytes()

    def flush(self) -> bool:
        return bool(lib().vsfh_group_flush(self._h))

    def queue_stats(self) -> dict:
        """vsf_observe_stats of the group's context, by name (capi.Context.observe_stats)."""
        v = np.zeros(len(capi.OBSERVE_STATS), np.int64)
        st = lib().vsfh_group_queue_stats(self._h, _p(v), len(v))
        if st != capi.VSF_OK:
            raise capi.VsfError(st, "vsf_observe_stats")
        return {k: int(x) for k, x in zip(capi.OBSERVE_STATS, v)}

    def close(self):
        if getattr(self, "_h", None):
            lib().vsfh_group_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
