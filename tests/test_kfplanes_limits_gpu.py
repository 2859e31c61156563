"""msl_keyframe_planes and msl_manhattan_observe at the limits their ABI accepts: pcap = 64 with 64 distinct held rows whose normals are so
short that every dot product passes the gate -- C(64, 3) = 41 664 triples and 2 016 pairs, the most a keyframe can add -- into empty
tables at fcap = qcap = 65536 and into tables pre-filled with 30 000 foreign keys (the triples no longer fit: NO_ROOM, bytes untouched; the
pairs do); mcap = kcap = 4096 with the held rows, the new rows and the keyframe row at the top of their range; n_frames = 1.  Every in/out
array and output against tests/kfplanes_model.py, as bytes, in device memory under guard bands."""
import numpy as np
import pytest

from tests import kfplanes_model as kp
from tests import kfplanes_scenes as ks
from tests.test_kfplanes_gpu import differences, matcher, run  # noqa: F401  (matcher: the module's fixture)

pytestmark = pytest.mark.gpu
PCAP, MCAP, FCAP, QCAP, KCAP = 64, 4096, 65536, 65536, 4096
CAPS = (PCAP, MCAP, FCAP, QCAP, KCAP)


def limit_frame(prefill, n_new=0):
    """64 planes with normals of length <= 0.1, the first 64 - n_new held on distinct rows at the top of a map of 4096 - n_new rows."""
    rng = np.random.default_rng(9200 + prefill)
    n_map = MCAP - n_new
    f = ks.frame(rng, PCAP, n_map, slot=KCAP - 1, kf_id=2 ** 31 - 1, n_kf=0)
    f["plane_coef"][:, :3] = rng.uniform(-0.05, 0.05, (PCAP, 3)).astype(np.float32)
    f["plane_match"][:PCAP - n_new, 0] = rng.permutation(np.arange(n_map - 200, n_map))[:PCAP - n_new]
    if prefill:                                                                # foreign keys all over the map: no key whose rows are all held,
        held = np.sort(f["plane_match"][:, 0])                                 # but five triples and three pairs the keyframe names itself
        for w, own, name in ((3, held[:15].reshape(3, 5).T, "full"), (2, held[20:26].reshape(2, 3).T, "part")):
            keys = np.sort(rng.integers(0, MCAP, (prefill + 3000, w)), 1)
            keys = keys[(np.diff(keys, axis=1) > 0).all(1) & ~np.isin(keys, held).all(1)]
            keys = np.concatenate([own, keys])
            f[name] = ks.unique(np.concatenate([keys, np.ones((len(keys), w + 1), np.int64)], 1), w)[:prefill]
    return f


@pytest.mark.parametrize("prefill", [0, 30000])
def test_the_most_keys_a_keyframe_can_add(matcher, prefill):
    from manhattanslam_amd import kfplanes
    _, a = kfplanes.pack([limit_frame(prefill)], *CAPS)
    want = ks.expected(a, kp.KEYFRAME, fill=ks.host_filled)
    *got, intact = run(a, kp.KEYFRAME, "device", matcher, CAPS)
    got[0].pop("kf_plane_match")
    assert differences(got, want, a["n_planes"], True) == [] and intact
    oo, nf = want[2], int(a["n_full"][0])
    assert oo["added_part"][0] == (2013 if prefill else 2016) and want[0]["n_part"][0] == a["n_part"][0] + oo["added_part"][0]
    if prefill:
        assert nf > FCAP - 41664 and oo["added_full"][0] == 0 and oo["status"][0] == kp.FULL_NO_ROOM and oo["set_not_erase"][0] == 1
        assert want[0]["full_tab"].tobytes() == a["full_tab"].tobytes() and want[0]["n_full"][0] == nf
    else:
        assert oo["added_full"][0] == 41664 == want[0]["n_full"][0] and oo["status"][0] == 0


def test_rows_at_the_top_of_the_map_and_keyframe_tables(matcher):
    """n_frames = 1, mcap = kcap = 4096: the last five planes become rows 4091 .. 4095, the keyframe is row 4095, kf_id is INT_MAX."""
    from manhattanslam_amd import kfplanes
    _, a = kfplanes.pack([limit_frame(0, n_new=5)], *CAPS)
    want = ks.expected(a, kp.KEYFRAME, fill=ks.host_filled)
    *got, intact = run(a, kp.KEYFRAME, "device", matcher, CAPS)
    got[0].pop("kf_plane_match")
    assert differences(got, want, a["n_planes"], True) == [] and intact
    assert want[1]["merge_into"][0, 59:].tolist() == list(range(4091, 4096)) and want[0]["n_map"][0] == 4096
    assert (want[0]["mp_first_kf"][0, 4091:] == 2 ** 31 - 1).all() and want[2]["recent_plane"][0, 59:].all() and want[2]["added_full"][0] == 41664
    a["n_map"][0] = 4094                                                       # two rows left for five planes
    a["plane_match"][0, :59, 0] = np.minimum(a["plane_match"][0, :59, 0], 4093)
    want = ks.expected(a, kp.KEYFRAME, fill=ks.host_filled)
    *got, intact = run(a, kp.KEYFRAME, "device", matcher, CAPS)
    got[0].pop("kf_plane_match")
    assert differences(got, want, a["n_planes"], True) == [] and intact
    assert want[1]["status"][0, 59:].tolist() == [kp.NEW, kp.NEW, kp.NO_ROOM, kp.NO_ROOM, kp.NO_ROOM]
