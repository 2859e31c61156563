"""The inputs of the FP64 group-sum checks, the same numbers tests/sp_arith_host.cpp generates (group_input): value k of lane l of group q is a
double with sign, exponent -40 .. 40 and mantissa taken from splitmix64 of the element's number, so that the partial sums round and the order of
the additions shows in the result's bits.  Plus array models of the DPP row operations the kernels use."""
import numpy as np

GROUPS = 2048   # groups per kind (4 and 10 values) the host program checks; a GPU test may use the first few


def splitmix(i):
    with np.errstate(over="ignore"):
        z = (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def group_inputs(groups, nvals):
    """[groups][nvals][16] doubles."""
    q = np.arange(groups, dtype=np.uint64)[:, None, None]
    k = np.arange(nvals, dtype=np.uint64)[None, :, None]
    l = np.arange(16, dtype=np.uint64)[None, None, :]
    z = splitmix(((q * np.uint64(16) + np.uint64(nvals)) * np.uint64(16) + k) * np.uint64(16) + l)
    e = np.uint64(1023 - 40) + (z >> np.uint64(1)) % np.uint64(81)
    bits = ((z & np.uint64(1)) << np.uint64(63)) | (e << np.uint64(52)) | (z >> np.uint64(12))
    return np.ascontiguousarray(bits).view(np.float64)


def checksum(groups=GROUPS):
    """What sp_arith_host prints as `groups checksum`: sum over all inputs of bits * (2 lane + 1), mod 2^64."""
    w = (2 * np.arange(16, dtype=np.uint64) + np.uint64(1))[None, None, :]
    with np.errstate(over="ignore"):
        return int(sum((group_inputs(groups, n).view(np.uint64) * w).sum(dtype=np.uint64) for n in (4, 10)) & np.uint64(0xFFFFFFFFFFFFFFFF))


def ror(v, n):
    """row_ror:n over the last axis (16 lanes): lane i receives lane i - n."""
    return np.roll(v, n, axis=-1)


def butterfly(v):
    """The one-value group sum over the last axis, every lane receiving the total: row_ror:8, row_ror:4, quad_perm [2,3,0,1], quad_perm [1,0,3,2]."""
    lanes = np.arange(16)
    v = v + ror(v, 8)
    v = v + ror(v, 4)
    v = v + v[..., lanes ^ 2]
    return v + v[..., lanes ^ 1]
