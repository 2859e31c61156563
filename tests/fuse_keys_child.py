"""Child process of tests/test_valu_diet_gpu.py: one resident call of nine keyframes on a 1 024- and an 8 192-surfel map, under the map-chain
switches of the environment it is started with (MSL_SF_DEFER, MSL_SF_DEAL: read once per process).  Writes the downloaded maps, the screen keys
k_fuse left, the dealing table and the chain counters to the .npz named on the command line.

The maps are laid out so that the keys tell WHICH keyframe wrote them: sub-blocks (128 surfels) alternate between surfels seen by keyframes
0 .. 7 only (even sub-blocks) and surfels seen by keyframe 8 only (odd ones; keyframe 8 looks 80 degrees to the side).  Half of each map is
therefore in view of every keyframe, and the keys of keyframe 8 are < 255 on the odd sub-blocks and 255 on the even ones -- the reverse of the
keys any earlier keyframe leaves."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, NKF, K_LAST = 640, 480, 9, 160
SIZES = (1024, 8192)


def frame_numbers():
    return list(range(NKF - 1)) + [K_LAST]


def in_image(m, pose, margin):
    """float64 projection of the surfels with a column-major Twc; inside the image shrunk by `margin` pixels (negative: grown) and inside the
    depth range shrunk (grown) likewise"""
    from manhattanslam_amd import synth
    I = synth.TUM1
    T = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4).T)
    p = np.stack([m["px"], m["py"], m["pz"], np.ones(len(m))], axis=1).astype(np.float64) @ T.T
    z = p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = p[:, 0] * I["fx"] / z + I["cx"], p[:, 1] * I["fy"] / z + I["cy"]
    dz = 0.1 if margin > 0 else -0.1
    return (z > 0.5 + dz) & (z < 30.0 - dz) & (u >= 1 + margin) & (u <= W - 2 - margin) & (v >= 1 + margin) & (v <= H - 2 - margin)


def inputs(n):
    """(map of n surfels, [(gray, depth, member, pose)] * 9)"""
    from manhattanslam_amd import synth, SURFEL_DTYPE
    ks = frame_numbers()
    frames = [synth.surfel_frame(k, variant="B" if i == 2 else "A") for i, k in enumerate(ks)]
    pool = synth.surfel_map(24 * n, ref=0, seed=23).astype(SURFEL_DTYPE)
    first = np.ones(len(pool), bool)
    any_first = np.zeros(len(pool), bool)
    for f in frames[:-1]:
        first &= in_image(pool, f[3], 12)
        any_first |= in_image(pool, f[3], -40)
    last, any_last = in_image(pool, frames[-1][3], 12), in_image(pool, frames[-1][3], -40)
    a, b = pool[first & ~any_last], pool[last & ~any_first]
    half = n // 2
    assert len(a) >= half and len(b) >= half, (len(a), len(b))
    m = np.zeros(n, SURFEL_DTYPE)
    blocks = m.reshape(n // 128, 128)
    blocks[0::2] = a[:half].reshape(-1, 128)
    blocks[1::2] = b[:half].reshape(-1, 128)
    return m, frames


def main(out):
    from manhattanslam_amd import SurfelFusion, synth
    I = synth.TUM1
    res = {}
    for n in SIZES:
        m, frames = inputs(n)
        g = SurfelFusion(W, H, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
        g.set_batch_capacity(NKF)
        g.map_upload(m)
        g.fuse_resident_batch(np.arange(NKF), np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]),
                              [f[3] for f in frames])
        g.sync()
        G = int(g.debug_scratch(1, which=4)[0])
        nk = max(G, n // 128)
        res[f"G{n}"] = G
        res[f"keys{n}"] = g.debug_scratch(nk, which=2)
        res[f"table{n}"] = g.debug_scratch(max(G, 1), which=3)
        res[f"chain{n}"] = g.debug_scratch(2, which=5)
        res[f"map{n}"] = g.map_download()
        g.close()
    np.savez(out, **res)
    print("fuse_keys_child ok")


if __name__ == "__main__":
    main(sys.argv[1])
