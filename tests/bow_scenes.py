"""Synthetic vocabularies and keyframe / frame pairs for the bag-of-words tests, generated at run time (no vocabulary file is committed).

Vocabularies are argument tuples of bow_model.build / manhattanslam_amd.bow.Vocabulary: (k, L, scoring, weighting, parent, is_leaf, desc,
weight), nodes in file order (a parent before its children)."""
import numpy as np


def random_vocab(seed, k=6, L=4, scoring=0, weighting=0, p_child=0.85, p_unflag=0.1, p_zero=0.1, p_dup=0.15):
    """An uneven tree: a node above level L gets 1..k children with probability p_child (shallow leaves otherwise); childless nodes are
    flagged except with probability p_unflag; weights are 0 (stopped) with probability p_zero; a child copies an earlier sibling's
    descriptor with probability p_dup (ties)."""
    rng = np.random.default_rng(seed)
    parent, depth = [0], [0]
    frontier = [0]
    order_children = {0: []}
    while frontier:
        nxt = []
        for nd in frontier:
            if depth[nd] >= L or (nd != 0 and rng.random() > p_child):
                continue
            for _ in range(int(rng.integers(1 if nd else 2, k + 1))):
                i = len(parent)
                parent.append(nd)
                depth.append(depth[nd] + 1)
                order_children.setdefault(nd, []).append(i)
                nxt.append(i)
        frontier = nxt
    n = len(parent)
    has_child = np.zeros(n, bool)
    has_child[np.array(parent[1:], np.int64)] = True
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for sibs in order_children.values():
        for j in range(1, len(sibs)):
            if rng.random() < p_dup:
                desc[sibs[j]] = desc[sibs[int(rng.integers(0, j))]]
    is_leaf = (~has_child & (rng.random(n) >= p_unflag)).astype(np.uint8)
    is_leaf[0] = 0
    weight = rng.uniform(0.05, 3.0, n)
    weight[rng.random(n) < p_zero] = 0.0
    return k, L, scoring, weighting, np.array(parent, np.int32), is_leaf, desc, weight


def full_vocab(seed, k=10, L=6, scoring=0, weighting=0, p_zero=0.02):
    """A full k-ary tree of depth L in breadth-first file order: ORBvoc's shape for k = 10, L = 6 (1 111 111 nodes)."""
    rng = np.random.default_rng(seed)
    n = (k ** (L + 1) - 1) // (k - 1)
    parent = np.zeros(n, np.int32)
    parent[1:] = (np.arange(1, n) - 1) // k
    first_leaf = (k ** L - 1) // (k - 1)
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[first_leaf:] = 1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = rng.uniform(0.1, 5.0, n)
    weight[rng.random(n) < p_zero] = 0.0
    return k, L, scoring, weighting, parent, is_leaf, desc, weight


def flip_bits(rng, d, nbits):
    """A copy of the 32-byte descriptors d with nbits random bits flipped per row."""
    d = np.array(d, np.uint8, copy=True).reshape(-1, 32)
    for r in range(len(d)):
        for b in rng.choice(256, nbits, replace=False):
            d[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def frame_descs(seed, vocab, n, noise=12):
    """n descriptors near the vocabulary's node descriptors (noisy copies), so descents spread over the tree, plus random ones."""
    rng = np.random.default_rng(seed)
    desc = vocab[6]
    base = desc[rng.integers(1, len(desc), n)] if len(desc) > 1 else rng.integers(0, 256, (n, 32), dtype=np.uint8)
    out = flip_bits(rng, base, noise) if n else np.zeros((0, 32), np.uint8)
    rnd = rng.random(n) < 0.2
    out[rnd] = rng.integers(0, 256, (int(rnd.sum()), 32), dtype=np.uint8)
    return out


def bow_pair(seed, n_kf, n_cur, n_nodes=6, rot=25.0, noise=6):
    """A keyframe / frame pair for SearchByBoW: frame features are noisy copies of keyframe features (a few rotated off the main bin),
    plus distractors and exact duplicates (ties); node ids from a small set so nodes hold many features (> 64 when n is large)."""
    rng = np.random.default_rng(seed)
    kf = rng.integers(0, 256, (n_kf, 32), dtype=np.uint8)
    src = rng.integers(0, max(n_kf, 1), n_cur) if n_kf else np.zeros(n_cur, np.int64)
    cur = flip_bits(rng, kf[src], noise) if n_kf and n_cur else rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    dist = rng.random(n_cur) < 0.25
    cur[dist] = rng.integers(0, 256, (int(dist.sum()), 32), dtype=np.uint8)
    dup = np.flatnonzero(rng.random(n_cur) < 0.05)
    for i in dup:
        if i > 0:
            cur[i] = cur[i - 1]
    kf_node = rng.integers(0, n_nodes, n_kf).astype(np.int32)
    kf_node[rng.random(n_kf) < 0.05] = -1
    cur_node = kf_node[src].copy() if n_kf else rng.integers(0, n_nodes, n_cur).astype(np.int32)
    moved = rng.random(n_cur) < 0.1
    cur_node[moved] = rng.integers(-1, n_nodes, int(moved.sum()))
    kf_angle = rng.uniform(0, 360, n_kf).astype(np.float32)
    cur_angle = ((kf_angle[src] if n_kf else rng.uniform(0, 360, n_cur)) - rot + rng.normal(0, 3, n_cur)).astype(np.float32) % np.float32(360)
    off = rng.random(n_cur) < 0.1
    cur_angle[off] = rng.uniform(0, 360, int(off.sum())).astype(np.float32)
    kf_flags = (rng.random(n_kf) < 0.85).astype(np.uint8)
    return {"kf_desc": kf, "kf_angle": kf_angle, "kf_node": kf_node, "kf_flags": kf_flags, "cur_angle": cur_angle.astype(np.float32),
            "cur_desc": cur, "cur_node": cur_node.astype(np.int32)}


def line_pair(seed, n_kf, n_cur, noise=10):
    """A keyframe / frame pair for SearchByDescriptor: current lines are noisy copies of keyframe lines (permuted) plus distractors and
    duplicates (ties); some keyframe lines hold no map line; world positions for the pose layout."""
    rng = np.random.default_rng(seed)
    kf = rng.integers(0, 256, (n_kf, 32), dtype=np.uint8)
    cur = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    if n_kf:
        m = min(n_kf, n_cur)
        idx = rng.permutation(n_cur)[:m]
        cur[idx] = flip_bits(rng, kf[rng.integers(0, n_kf, m)], noise)
    for i in np.flatnonzero(rng.random(n_cur) < 0.08):
        cur[i] = cur[int(rng.integers(0, n_cur))]
    return {"kf_ldesc": kf, "kf_flags": (rng.random(n_kf) < 0.8).astype(np.uint8), "kf_xyz": rng.normal(0, 2, (n_kf, 6)), "cur_ldesc": cur}
