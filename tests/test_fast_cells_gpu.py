"""k_fast (one wave per FAST cell, packed quick test, iniTh then minTh) against the CPU oracle on small frames whose cell plans hold every kind
of cell the kernel treats differently: FAST candidates of every level (coordinates, responses and order) and the full extraction, bit for bit.
Every constructed input is first checked against the oracle alone: a case the reference leaves empty would prove nothing."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INI_TH, MIN_TH = 20, 7
# name -> (width, height, levels).  "small": 156 x 120, levels 156 / 130 / 108 / 90 wide: 31-px cells, one 58-px-wide cell on the last level.
# "strip": 783 x 100: 25 columns of 31 px leave a last column that is 1 px wide on level 0.
GEOMETRIES = {"small": (156, 120, 4), "strip": (783, 100, 3)}


def axis_cells(n):
    """Cells along one axis of a level that is n pixels long (src/ORBextractor.cc:728-743): [(first FAST pixel, extent)], skipped cells left out."""
    lo, hi = 16, n - 16
    count = int(float(hi - lo) / 30)
    size = int(math.ceil(float(hi - lo) / count))
    out = []
    for j in range(count):
        ini = lo + j * size
        if ini >= hi - 6:   # (the reference's test for rows is hi - 3: such a row has no extent either)
            continue
        ext = min(ini + size + 6, hi) - ini - 6
        if ext > 0:
            out.append((ini + 3, ext))
    return size, out


def cell_plan(level_shapes):
    """[(cell pitch x, cell pitch y, column cells, row cells)] per level."""
    plan = []
    for h, w in level_shapes:
        sx, cols = axis_cells(w)
        sy, rows = axis_cells(h)
        plan.append((sx, sy, cols, rows))
    return plan


def _value_texture(rng, h, w, lo, hi, block):
    """Blocks of block x block pixels with random values in [lo, hi]."""
    g = rng.integers(lo, hi + 1, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    return np.kron(g, np.ones((block, block), np.uint8))[:h, :w].copy()


def make_image(kind, w, h):
    rng = np.random.default_rng(20261018)
    if kind == "constant":
        return np.full((h, w), 90, np.uint8)
    if kind == "noise":          # nearly every pixel passes the quick test: far more than 256 candidates in a 31 x 44 cell
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "fallback":       # two grey levels 12 apart: every difference between two pixels is 0 or 12, inside (7, 20)
        return np.where(_value_texture(rng, h, w, 0, 1, 3) > 0, 112, 100).astype(np.uint8)
    if kind == "mixed":          # strong texture on the left, the two-level texture on the right: only the cells on the right fall back
        img = np.where(_value_texture(rng, h, w, 0, 1, 3) > 0, 112, 100).astype(np.uint8)
        img[:, :w // 2] = _value_texture(rng, h, w // 2, 0, 255, 3)
        return img
    if kind == "tie":
        # level 0, cell (row 0, column 1): flat but for two adjacent pixels 50 above it (both score 49 and neither is a strict maximum: nothing
        # is kept at 20 although scores >= 20 exist) and one lone pixel 12 above it (scores 11: kept at 7)
        img = _value_texture(rng, h, w, 0, 255, 4)
        (_, _, cols, rows), = cell_plan([(h, w)])
        (x0, cw), (y0, ch) = cols[1], rows[0]
        img[y0 - 3:y0 + ch + 3, x0 - 3:x0 + cw + 3] = 100
        img[y0 + 10, x0 + 8:x0 + 10] = 150
        img[y0 + 25, x0 + 20] = 112
        return img
    raise KeyError(kind)


_oracle_runs = {}


def oracle_run(oracle, geom, kind):
    """(image, keypoints, descriptors, [candidates per level], level shapes) of the oracle, computed once and read-only."""
    if (geom, kind) not in _oracle_runs:
        w, h, levels = GEOMETRIES[geom]
        img = make_image(kind, w, h)
        oex = oracle.orb_create(500, 1.2, levels, INI_TH, MIN_TH)
        k, d = oex.extract(img)
        cands = [oex.candidates(l) for l in range(levels)]
        shapes = [(h, w)] + [oex.level(l).shape for l in range(1, levels)]
        for a in [img, k, d] + cands:
            a.flags.writeable = False
        _oracle_runs[(geom, kind)] = (img, k, d, cands, shapes)
    return _oracle_runs[(geom, kind)]


def in_cell(cands, x0, cw, y0, ch):
    """Candidates (x, y, response; level coordinates) of one cell."""
    x, y = cands[:, 0], cands[:, 1]
    return cands[(x >= x0) & (x < x0 + cw) & (y >= y0) & (y < y0 + ch)]


def check_input_against_oracle(geom, kind, run):
    """What the input is meant to provoke happens in the oracle."""
    img, k, d, cands, shapes = run
    plan = cell_plan(shapes)
    if kind == "constant":
        assert len(k) == 0 and all(len(c) == 0 for c in cands)
        return
    assert all(len(c) > 0 for c in cands), [len(c) for c in cands]
    if kind == "noise":
        sx, sy, cols, rows = plan[0]
        (x0, cw), (y0, ch) = cols[0], rows[0]
        region = img[y0 - 3:y0 + ch + 3, x0 - 3:x0 + cw + 3].astype(np.int32)
        c = region[3:-3, 3:-3]
        ring = lambda dx, dy: region[3 + dy:3 + dy + ch, 3 + dx:3 + dx + cw]
        pairs = [(ring(0, 3), ring(0, -3)), (ring(3, 0), ring(-3, 0)), (ring(2, 2), ring(-2, -2)), (ring(2, -2), ring(-2, 2))]
        # the quick test at iniTh: every opposite pair has a member darker than the centre by more than the threshold, or every pair a brighter one
        passing = np.all([(c - a > INI_TH) | (c - b > INI_TH) for a, b in pairs], axis=0) | np.all([(a - c > INI_TH) | (b - c > INI_TH) for a, b in pairs], axis=0)
        print("noise: cell 0 of level 0 is %d x %d, %d pixels pass the quick test at %d" % (cw, ch, passing.sum(), INI_TH))
        assert passing.sum() > 256
    if kind == "fallback":   # every kept corner is below iniTh: every cell that holds one fell back
        assert all((c[:, 2] >= MIN_TH).all() and (c[:, 2] < INI_TH).all() for c in cands)
        for l, (sx, sy, cols, rows) in enumerate(plan):
            filled = [len(in_cell(cands[l], x0, cw, y0, ch)) > 0 for x0, cw in cols for y0, ch in rows]
            print("fallback: level %d, %d of %d cells keep corners below %d" % (l, sum(filled), len(filled), INI_TH))
            assert 4 * sum(filled) >= 3 * len(filled), l
    if kind == "mixed":
        r = cands[0][:, 2]
        assert (r >= INI_TH).any() and (r < INI_TH).any()
    if kind == "tie":
        _, _, cols, rows = plan[0]
        (x0, cw), (y0, ch) = cols[1], rows[0]
        got = in_cell(cands[0], x0, cw, y0, ch)
        assert got.tolist() == [[x0 + 20, y0 + 25, 11]], got


def print_plan(geom, shapes):
    plan = cell_plan(shapes)
    for l, (sx, sy, cols, rows) in enumerate(plan):
        print("%s level %d %dx%d: cell pitch %dx%d, widths %s, heights %s" % (geom, l, shapes[l][1], shapes[l][0], sx, sy, [c[1] for c in cols], [r[1] for r in rows]))
    return plan


def test_plans_hold_every_cell_class(oracle):
    """The geometries above contain: a one-column level whose cell is wider than 56 px, ordinary 30-31 px cells, and a last column narrower
    than 4 px (the quick test's groups of four pixels are masked there)."""
    small = print_plan("small", oracle_run(oracle, "small", "constant")[4])
    strip = print_plan("strip", oracle_run(oracle, "strip", "constant")[4])
    assert any(len(cols) == 1 and sx > 56 for sx, _, cols, _ in small)   # (58-px cell; the level's right border leaves 52 px of it)
    assert any(30 <= cw <= 31 for _, _, cols, _ in small for _, cw in cols)
    assert any(0 < cols[-1][1] < 4 for _, _, cols, _ in strip)
    assert any(cw % 4 for _, _, cols, _ in small for _, cw in cols)      # widths that are no multiple of the group
    assert any(len(rows) > 1 for _, _, _, rows in small)                 # more than one cell row


def _assert_same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    assert kg.tobytes() == ko.tobytes()
    if len(kg):
        assert np.array_equal(dg, do)
    else:
        assert dg is None or len(dg) == 0


@pytest.fixture(scope="module")
def extractors():
    from manhattanslam_amd import ORBextractor
    made = {g: ORBextractor(500, 1.2, L, INI_TH, MIN_TH, max_width=w, max_height=h, max_batch=8) for g, (w, h, L) in GEOMETRIES.items()}
    yield made
    for ex in made.values():
        ex.close()


@pytest.mark.parametrize("kind", ["constant", "noise", "fallback", "mixed", "tie"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_cells_match_oracle(extractors, oracle, geom, kind):
    run = oracle_run(oracle, geom, kind)
    check_input_against_oracle(geom, kind, run)
    img, ko, do, cands, shapes = run
    ex = extractors[geom]
    kg, dg = ex(img)
    for l in range(len(cands)):
        assert ex.level_size(l) == (shapes[l][1], shapes[l][0])
        got = ex.debug_candidates(0, l)
        assert np.array_equal(got, cands[l]), (l, len(got), len(cands[l]))
    _assert_same(kg, dg, ko, do)


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_batch_of_different_frames_equals_single_calls(extractors, oracle, geom):
    kinds = ["noise", "tie", "constant", "fallback", "mixed", "tie", "fallback", "noise"]
    runs = [oracle_run(oracle, geom, k) for k in kinds]
    imgs = np.stack([r[0] for r in runs])
    imgs[5] = imgs[5][::-1, ::-1]          # eight different frames
    imgs[6] = np.roll(imgs[6], 5, axis=1)
    imgs[7] = 255 - imgs[7]
    ex = extractors[geom]
    singles = [ex(im) for im in imgs]
    single_cands = []
    for im in imgs:
        ex(im)
        single_cands.append([ex.debug_candidates(0, l) for l in range(GEOMETRIES[geom][2])])
    batch = ex.extract_batch(imgs)
    assert len({im.tobytes() for im in imgs}) == 8
    for f in range(8):
        _assert_same(batch[f][0], batch[f][1], singles[f][0], singles[f][1] if singles[f][1] is not None else np.zeros((0, 32), np.uint8))
        for l in range(GEOMETRIES[geom][2]):
            assert np.array_equal(ex.debug_candidates(f, l), single_cands[f][l]), (f, l)
        if f < 5:   # the unmodified frames: the oracle's result as well
            _assert_same(batch[f][0], batch[f][1], runs[f][1], runs[f][2])
