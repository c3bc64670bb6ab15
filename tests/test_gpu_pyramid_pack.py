"""Pyramid lane packing: a band narrower than a wave has the lane spans of neighbouring strips packed into full waves
(resize_strip_kernel's last band, pyramid_image_kernel's narrow levels).  Every level of the first and of the last image
of a batch, byte for byte against the oracle, for batches that take the per-level launches alone (20 images) and the
per-level launches plus the image-major tail (the smallest batch that fills the CUs), at sizes that put a level's width
on every packing boundary, for the 50-level / 1.04 pyramid and the 8-level / 1.2 one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# size -> a width that some level >= 1 of the 1.04 pyramid must have (None: no such demand)
#   256: one full band, nothing to pack; 257 / 260: a second band of 1 / 4 columns (257: a partial last lane);
#   512: two full bands; heights of 45 and 77 end in levels shorter than one 8-row strip and one 16-row strip;
#   640x480: the benchmark's shape (last bands of 103 ... 4 columns, tail levels of 250 ... 94)
SIZES = [((640, 480), 615), ((266, 203), 256), ((267, 45), 257), ((270, 131), 260), ((532, 77), 512),
         ((333, 217), None), ((97, 61), None)]
PYRAMIDS = [dict(), dict(scale_factor=1.2, nlevels=8)]


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _tail_batch():
    """The smallest batch for which vsf_launch_pyramid hands the one-band levels to pyramid_image_kernel: at least 64
    images and a last round of workgroups at least three quarters of the CUs."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return max(64, (3 * ncu + 3) // 4)


def _image(base, i):
    """Image i of the batch: every one different (shifted and with its own grey offset)."""
    return np.ascontiguousarray(np.roll(base, (3 * i, 5 * i), axis=(0, 1)) ^ np.uint8((37 * i) & 0xFF))


_oracle_levels = {}


def _reference(oracle, base, size, pi, i, nlevels):
    key = (size, pi, i)
    if key not in _oracle_levels:
        o = oracle.Orb(nfeatures=300, **PYRAMIDS[pi])
        o.run(_image(base, i))
        _oracle_levels[key] = [o.level_image(l, False).copy() for l in range(nlevels)]
    return _oracle_levels[key]


@pytest.mark.parametrize("batch", ["20", "tail"])
@pytest.mark.parametrize("pi", [0, 1], ids=["50x1.04", "8x1.2"])
@pytest.mark.parametrize("size,want_width", SIZES, ids=["%dx%d" % s for s, _ in SIZES])
def test_packed_pyramid_levels_bit_exact(capi, oracle, size, want_width, pi, batch):
    import torch
    from vision_slam_frontend_amd import synth
    w, h = size
    n = 20 if batch == "20" else _tail_batch()
    dev = torch.device("cuda", 0)
    p = capi.default_params(w, h, max_images=n, nfeatures=300)
    for k, v in PYRAMIDS[pi].items():
        setattr(p, k, v)
    base = synth.stereo_pair(w, h, 11, n_objects=200)[0]
    with capi.Context(p) as ctx:
        widths = [ctx.level_info(l)[0] for l in range(ctx.nlevels)]
        if pi == 0 and want_width is not None:
            assert want_width in widths[1:], widths
        K = int(ctx.params.max_keypoints)
        pitch = (w + 15) // 16 * 16
        padded = np.zeros((n, h, pitch), np.uint8)
        for i in range(n):
            padded[i, :, :w] = _image(base, i)
        d = torch.from_numpy(padded).to(dev)
        kp = torch.zeros((n, K, 28), dtype=torch.uint8, device=dev)
        de = torch.zeros((n, K, 32), dtype=torch.uint8, device=dev)
        cn = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.extract_batch_dev(d.data_ptr(), n, pitch * h, pitch, kp.data_ptr(), de.data_ptr(), cn.data_ptr())
        ctx.sync(allow_capacity=True)
        for i in (0, n - 1):
            ref = _reference(oracle, base, size, pi, i, ctx.nlevels)
            for l in range(ctx.nlevels):
                np.testing.assert_array_equal(ctx.debug_level_image(i, l, False), ref[l],
                                              err_msg="%dx%d n=%d image %d level %d (width %d)" % (w, h, n, i, l, widths[l]))
