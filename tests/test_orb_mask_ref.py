"""Pins tests/orb_mask_ref.py (the reference of the GPU mask tests) against the unmodified CPU oracle, and checks that the scenes
those tests use exercise the feature.  No GPU.

1. the pin: with the filter skipped, and with an all-255 mask, the reference reproduces vsfo_orb_result bit for bit on every
   scene -- keypoints with response and angle as raw bits, descriptors.  This pins the Harris restatement and the composition
   of the two cuts;
2. every level of an all-255 mask is all 255; an all-254 mask is all 0 from level 1 on; a region erodes through the chained
   levels (level l is built from level l - 1: building it from level 0 gives another pyramid);
3. the scenes bite: the masked result differs from the unmasked one, at least one level still has more than 2 n_l candidates
   behind the filter (both cuts run on filtered lists), and on at least one level the masked result holds a corner the
   unmasked result does not hold (a slot the mask freed was refilled) -- in HARRIS and FAST_SCORE mode."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import orb_mask_ref as ref  # noqa: E402
from oracle import binding as ob  # noqa: E402

SCENES = ref.scenes()


def _oracle_result(img, nfeatures, kw):
    o = ob.Orb(nfeatures=nfeatures, **kw)
    o.run(img)
    return o.result()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_without_the_filter_is_the_oracle(name):
    img, _, nfeatures, kw = SCENES[name]
    want_kp, want_desc = _oracle_result(img, nfeatures, kw)
    assert len(want_kp) > 15
    full = np.full(img.shape, 255, np.uint8)
    for what, got in (("filter skipped", ref.reference(img, full * 0, nfeatures, ref.HARRIS, skip_filter=True, **kw)),
                      ("no mask", ref.reference(img, None, nfeatures, ref.HARRIS, **kw)),
                      ("all-255 mask", ref.reference(img, full, nfeatures, ref.HARRIS, **kw))):
        assert got[0].tobytes() == want_kp.tobytes(), "%s, %s: keypoints differ from the oracle's" % (name, what)
        assert np.array_equal(got[1], want_desc), "%s, %s: descriptors differ from the oracle's" % (name, what)
        assert sum(got[2]) == len(want_kp)


@pytest.mark.parametrize("size,kw", [((160, 120), ref.SMALL), ((97, 75), ref.SMALL), ((640, 480), dict())])
def test_mask_pyramid_rules(size, kw):
    w, h = size
    orb = ob.Orb(nfeatures=100, **kw)
    sizes = [info[:2] for info in orb.layout(w, h)]
    m = ref.masks(w, h)
    assert all((lv == 255).all() for lv in ref.mask_pyramid(m["all255"], sizes))
    p254 = ref.mask_pyramid(m["all254"], sizes)
    assert (p254[0] == 254).all() and all((lv == 0).all() for lv in p254[1:])
    for name, mask in m.items():
        for lv in ref.mask_pyramid(mask, sizes)[1:]:
            assert set(np.unique(lv)) <= {0, 255}, name
    # the chain: a level made from the thresholded level below loses ground that one made from level 0 would keep
    chained = ref.mask_pyramid(m["disc"], sizes)
    direct = [ref.tozero254(ob.resize_linear(m["disc"], sw, sh)) for sw, sh in sizes]
    lost = [int((direct[l] != 0).sum()) - int((chained[l] != 0).sum()) for l in range(2, len(sizes))]
    assert min(lost) >= 0 and max(lost) > 0, lost


@pytest.mark.parametrize("mode", [ref.HARRIS, ref.FAST_SCORE])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_bite(name, mode):
    img, mask, nfeatures, kw = SCENES[name]
    differs, crowded, refilled = ref.bites(img, mask, nfeatures, mode, **kw)
    print("%s mode %d: crowded levels %s, refilled levels %s" % (name, mode, crowded, refilled))
    assert differs, "the mask changes nothing"
    assert crowded, "no level keeps more than 2 n_l candidates behind the filter"
    assert refilled, "no slot freed by the mask was refilled"


def test_filter_is_a_predicate_on_the_raster_order_list():
    img, mask, nfeatures, kw = SCENES["noise160_half"]
    orb = ref.run_oracle(img, nfeatures, **kw)
    pyr = ref.mask_pyramid(mask, ref.level_sizes(orb))
    for level in range(orb.nlevels):
        s0 = orb.stage(0, level)
        kept = ref.filter_by_mask(s0, pyr[level])
        key = kept["y"].astype(np.int64) * 4096 + kept["x"].astype(np.int64)
        assert (np.diff(key) > 0).all()  # still raster order
        assert len(kept) <= len(s0)
    assert len(ref.filter_by_mask(orb.stage(0, 0), pyr[0])) < len(orb.stage(0, 0))
