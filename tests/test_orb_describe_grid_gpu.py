"""k_describe launches one wave per OUTPUT keypoint: a wave finds its level and its place in the level's selection from the running sums of the
frame's per-level counts.  Keypoints and descriptors against the CPU oracle, bit for bit, where that search can go wrong: no keypoint at all,
empty levels before and after the only level that has any, a total that is no multiple of the four waves of a workgroup, more keypoints than
nfeatures + 2 levels, and a batch whose frames have different totals (one of them none)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assert_same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    assert kg.tobytes() == ko.tobytes()
    if len(kg):
        assert np.array_equal(dg, do)
    else:
        assert dg is None or len(dg) == 0


def _blobs(w=1440, h=1080, sigma=5.0, amp=215.0):
    """Smooth bright blobs on a dark frame, for three levels a factor 4 apart and a FAST threshold of 60.  Level 0: a blob (sigma 5 px) has no
    step of 60 grey levels over the 3-px FAST ring.  Level 1: it is a peak of sigma 1.25 px, a corner.  Level 2 (90 x 68): the blobs lie in
    the top and bottom bands of the frame, outside the region its FAST cells cover."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.full((h, w), 20.0, np.float32)
    rng = np.random.default_rng(11)
    for y0 in (140, 200, 260, 860, 920):
        for x0 in range(160, 1300, 90):
            x, y = x0 + int(rng.integers(-8, 9)), y0 + int(rng.integers(-8, 9))
            sl = (slice(y - 30, y + 31), slice(x - 30, x + 31))
            img[sl] += amp * np.exp(-((xx[sl] - x) ** 2 + (yy[sl] - y) ** 2) / (2 * sigma * sigma))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def test_flat_image_has_no_keypoint_on_any_level(oracle):
    from manhattanslam_amd import ORBextractor
    flat = np.full((304, 400), 90, np.uint8)
    ex = ORBextractor(500, 1.2, 6, 25, 9, max_width=400, max_height=304)
    ko, do = oracle.orb_create(500, 1.2, 6, 25, 9).extract(flat)
    kg, dg = ex(flat)
    assert len(ko) == 0
    _assert_same(kg, dg, ko, do)
    ex.close()


def test_keypoints_on_the_middle_level_only(oracle):
    from manhattanslam_amd import ORBextractor
    img = _blobs()
    ex = ORBextractor(500, 4.0, 3, 60, 60, max_width=1440, max_height=1080)
    ko, do = oracle.orb_create(500, 4.0, 3, 60, 60).extract(img)
    assert len(ko) > 40 and set(ko["octave"]) == {1}          # levels 0 and 2 are empty
    kg, dg = ex(img)
    _assert_same(kg, dg, ko, do)
    ex.close()


def test_total_that_is_no_multiple_of_four(oracle):
    """Budgets of 50 and 52 features on a 400 x 304 frame return 63 and 66 keypoints: the last workgroup of four waves is part empty."""
    from manhattanslam_amd import ORBextractor, synth
    img = synth.orb_frame(4242, 400, 304)
    rests = set()
    for nf in (50, 52):
        ex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=400, max_height=304)
        ko, do = oracle.orb_create(nf, 1.2, 8, 20, 7).extract(img)
        rests.add(len(ko) % 4)
        kg, dg = ex(img)
        _assert_same(kg, dg, ko, do)
        ex.close()
    assert rests == {3, 2}


def test_more_keypoints_than_the_feature_budget(oracle):
    """The 1600 x 230, 300-feature geometry of test_quadtree_node_bound_over_geometries: seven quadtree roots per level, so the levels return more
    than nfeatures + 2 levels keypoints and the launch is sized by the capacity of the creation geometry."""
    from manhattanslam_amd import ORBextractor, synth
    w, h, nf, levels = 1600, 230, 300, 6
    img = synth.orb_frame(300 + w + nf, 1920, 1440)[:h, :w].copy()
    ex = ORBextractor(nf, 1.2, levels, 9, 5, max_width=w, max_height=h)
    ko, do = oracle.orb_create(nf, 1.2, levels, 9, 5).extract(img)
    assert len(ko) > nf + 2 * levels and ex.capacity >= len(ko)
    kg, dg = ex(img)
    _assert_same(kg, dg, ko, do)
    ex.close()


def test_batch_of_frames_with_different_totals(oracle):
    from manhattanslam_amd import ORBextractor, synth
    full = synth.orb_frame(4243)
    imgs = np.stack([full[:304, :400], np.full((304, 400), 200, np.uint8), full[150:454, 200:600]])
    imgs[2, :, 120:] = 128          # mostly flat: fewer keypoints than the budget
    ex = ORBextractor(300, 1.2, 6, 25, 9, max_width=400, max_height=304, max_batch=3)
    oex = oracle.orb_create(300, 1.2, 6, 25, 9)
    want = [oex.extract(np.ascontiguousarray(im)) for im in imgs]
    assert len(want[1][0]) == 0 and len(want[0][0]) > 0 and len(want[2][0]) > 0 and len(want[0][0]) != len(want[2][0])
    res = ex.extract_batch(imgs)
    for f in range(3):
        _assert_same(res[f][0], res[f][1], want[f][0], want[f][1])
    ex.close()
