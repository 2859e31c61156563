"""Seeded synthetic scenes for msl_pnp_ransac: a true pose, N non-coplanar points in front of the camera, pixel noise well under the
threshold on the inliers, a stated share of gross outliers, octaves spread over the levels and NULL matches interleaved.  The list of scenes
and seeds is fixed here; tests/test_pnp_model.py checks that every one of them keeps its inlier decisions 2^-19 away from the threshold."""
import numpy as np

NLEVELS, SCALE = 8, 1.2
FX = FY = 525.0
CX, CY = 319.5, 239.5


def pnp_scene(seed, N=120, kcap=160, n_null=10, outlier_share=0.3, sigma_px=0.2, all_outliers=False):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3); a *= 0.2 / np.linalg.norm(a)                                                  # small rotation vector
    K_ = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.linalg.norm(a)
    R = np.eye(3) + np.sin(th) / th * K_ + (1 - np.cos(th)) / th ** 2 * K_ @ K_
    t = rng.uniform(-0.3, 0.3, 3)
    Pc = np.stack([rng.uniform(-1.2, 1.2, N), rng.uniform(-0.9, 0.9, N), rng.uniform(1.5, 4.0, N)], 1)   # in front, non-coplanar
    Pw = (Pc - t) @ R                                                                                      # Pc = R Pw + t
    uv = np.stack([FX * Pc[:, 0] / Pc[:, 2] + CX, FY * Pc[:, 1] / Pc[:, 2] + CY], 1)
    uv += rng.normal(scale=sigma_px, size=uv.shape)
    out = np.ones(N, bool) if all_outliers else rng.random(N) < outlier_share
    uv[out] += rng.uniform(30, 120, (int(out.sum()), 2)) * rng.choice([-1, 1], (int(out.sum()), 2))        # gross outliers
    n_kps = N + n_null
    slot = np.sort(rng.choice(n_kps, N, replace=False))                                                    # keypoints holding a match
    match = np.full(n_kps, -1, np.int32); un_xy = rng.uniform(0, 480, (n_kps, 2)).astype(np.float32)
    if n_null:
        null = np.setdiff1d(np.arange(n_kps), slot)
        match[null[::2]] = 40000                                                                           # NULL is anything outside [0, kcap), whatever the batch's kcap
    kf_idx = rng.permutation(kcap)[:N].astype(np.int32)
    xyz = rng.normal(size=(kcap, 3)).astype(np.float32); xyz[kf_idx] = Pw.astype(np.float32)
    match[slot] = kf_idx; un_xy[slot] = uv.astype(np.float32)
    octave = rng.integers(0, NLEVELS, n_kps).astype(np.int32)
    Tcw = np.hstack([R, t[:, None]]).astype(np.float32)
    return dict(un_xy=un_xy, octave=octave, match=match, xyz=xyz, Tcw_true=Tcw, true_inlier=slot[~out], seed=np.uint32(seed), N=N)


def level_sigma2():
    return ((np.float32(SCALE) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)


def params_dict(max_iterations=40, n_iterations=5, min_inliers=10, epsilon=0.5, th2=5.991, probability=0.99, min_set=4):
    """The fields of msl_pnp_params (Tracking: (0.99, 10, 300, 4, 0.5, 5.991) and iterate(5))."""
    ls = np.zeros(16, np.float32); ls[:NLEVELS] = level_sigma2()
    return dict(fx=np.float32(FX), fy=np.float32(FY), cx=np.float32(CX), cy=np.float32(CY), nlevels=NLEVELS, level_sigma2=ls,
                probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, min_set=min_set, epsilon=np.float32(epsilon),
                th2=np.float32(th2), n_iterations=n_iterations)


# name -> (scene arguments, params arguments).  The seeds are fixed: test_pnp_model.py::test_margins holds them to the 2^-19 margin.
SCENES = {
    "empty":      (dict(seed=11, N=0, kcap=16, n_null=6), {}),
    "below":      (dict(seed=12, N=3, kcap=16, n_null=4), {}),
    "exact":      (dict(seed=13, N=10, kcap=24, n_null=5, outlier_share=0.0), {}),
    "eleven":     (dict(seed=14, N=11, kcap=24, n_null=5, outlier_share=0.0), {}),
    "ragged150":  (dict(seed=15, N=150, kcap=200, n_null=12, outlier_share=0.4), {}),
    "track_a":    (dict(seed=21, N=120, kcap=160, n_null=10, outlier_share=0.3), dict(max_iterations=300)),
    "track_b":    (dict(seed=23, N=120, kcap=160, n_null=10, outlier_share=0.3), dict(max_iterations=300)),
    "no_inliers": (dict(seed=31, N=60, kcap=80, n_null=8, all_outliers=True), {}),
    "full":       (dict(seed=44, N=8192, kcap=32768, n_null=0, outlier_share=0.1, sigma_px=0.05), dict(max_iterations=8)),
}
RAGGED = ("empty", "below", "exact", "eleven", "ragged150")

_cache = {}


def scene(name):
    """The named scene (built once, shared and left unchanged) and its params."""
    if name not in _cache:
        kw, pk = SCENES[name]
        _cache[name] = (pnp_scene(**kw), params_dict(**pk))
    return _cache[name]


_model = {}


def model(name):
    """The model's result for the named scene (computed once)."""
    if name not in _model:
        from . import pnp_model
        sc, p = scene(name)
        _model[name] = pnp_model.pnp_ransac(p, sc["octave"], sc["un_xy"], sc["match"], sc["xyz"], sc["seed"])
    return _model[name]
