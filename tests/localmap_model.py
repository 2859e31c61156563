"""The sequential model of msl_local_keyframes, msl_local_points and msl_local_lines: Tracking::UpdateLocalKeyFrames, UpdateLocalPoints /
UpdateLocalLines and the first loops of SearchLocalPoints / SearchLocalLines restated literally over Python objects -- dicts for the
counters, sets for the mnTrackReferenceForFrame / mnLastFrameSeen marks, pointer order replaced by table index -- and the reference's own
composition UpdateLocalMap -> SearchLocalPoints first loop.  Elements are named by their table index; None is NULL.

A scene (tests/localmap_scenes.py) is a dict:
  kf_bad [n_tab] bool      conn [n_tab] lists (mvpOrderedConnectedKeyFrames)      parent [n_tab] index or None
  held [n_tab] lists of point ids / None (mvpMapPoints of the keyframes)          lheld [n_tab] the same for lines
  pt_bad, pt_nobs [n_pts]; pt_obs [n_pts] lists of keyframe indices (mObservations' keys in iteration order)
  ln_bad, ln_nobs [n_lines]
  frames: list of dict(held, lheld: lists of ids / None; prev: the local keyframes on entry, a list)"""
NO_VOTES = 1
LOCAL_KF_STOP, BEST_COVIS = 80, 10


def update_local_keyframes(held, pt_bad, pt_obs, kf_bad, conn, parent, prev):
    """Tracking::UpdateLocalKeyFrames.  held is modified as the reference modifies mCurrentFrame.mvpMapPoints (bad points NULLed).
    Returns dict(votes: keyframeCounter, local_kf: mvpLocalKeyFrames, ref_kf: pKFmax or None (mpReferenceKF left alone), cleared: the
    slots NULLed, status)."""
    counter, cleared = {}, []
    for i in range(len(held)):
        if held[i] is not None:
            p = held[i]
            if not pt_bad[p]:
                for kf in pt_obs[p]:
                    counter[kf] = counter.get(kf, 0) + 1
            else:
                held[i] = None
                cleared.append(i)
    if not counter:
        return dict(votes=counter, local_kf=list(prev), ref_kf=None, cleared=cleared, status=NO_VOTES)
    mx, kfmax = 0, None
    local, mark = [], set()
    for kf in sorted(counter):                                        # map<KeyFrame*, int>: pointer order = table order
        if kf_bad[kf]:
            continue
        if counter[kf] > mx:
            mx, kfmax = counter[kf], kf
        local.append(kf)
        mark.add(kf)
    children = {}
    for c, p in enumerate(parent):
        if p is not None:
            children.setdefault(p, []).append(c)
    end = len(local)                                                  # itEndKF is taken before the loop
    for it in range(end):
        if len(local) > LOCAL_KF_STOP:
            break
        kf = local[it]
        for nb in conn[kf][:BEST_COVIS]:
            if not kf_bad[nb]:
                if nb not in mark:
                    local.append(nb)
                    mark.add(nb)
                    break
        for ch in sorted(children.get(kf, [])):                       # set<KeyFrame*>: pointer order = table order
            if not kf_bad[ch]:
                if ch not in mark:
                    local.append(ch)
                    mark.add(ch)
                    break
        p = parent[kf]
        if p is not None:
            if p not in mark:                                         # no isBad test
                local.append(p)
                mark.add(p)
                break                                                 # the outer loop's
    return dict(votes=counter, local_kf=local, ref_kf=kfmax, cleared=cleared, status=0)


def update_local_elements(local_kf, kf_held, bad):
    """Tracking::UpdateLocalPoints / UpdateLocalLines: mvpLocalMapPoints / mvpLocalMapLines."""
    local, mark = [], set()
    for kf in local_kf:
        for p in kf_held[kf]:
            if p is None:
                continue
            if p in mark:
                continue
            if not bad[p]:
                local.append(p)
                mark.add(p)
    return local


def search_first_loop(held, bad):
    """The first loop of SearchLocalPoints / SearchLocalLines: held is modified (bad elements NULLed); returns the set of elements whose
    mnLastFrameSeen is now the frame's."""
    seen = set()
    for i in range(len(held)):
        p = held[i]
        if p is not None:
            if bad[p]:
                held[i] = None
            else:
                seen.add(p)
    return seen


def element_flags(local, seen, nobs):
    """mp_flags / ml_flags: bit 0 candidate (every local element is !isBad()), bit 1 Observations() > 0."""
    return [(0 if p in seen else 1) | (2 if nobs[p] > 0 else 0) for p in local]


def held_flags(held, nobs):
    """cur_flags / cur_line_flags of the slots after the first loop."""
    return [0 if p is None else 1 | (2 if nobs[p] > 0 else 0) for p in held]


def update_local_map(scene, frame):
    """UpdateLocalMap followed by the first loops of SearchLocalPoints and SearchLocalLines for one frame of the scene, from the state on
    entry.  Returns dict(kf: update_local_keyframes' result, points / lines: dict(local, flags, cur_flags))."""
    held, lheld = list(frame["held"]), list(frame["lheld"])
    kf = update_local_keyframes(held, scene["pt_bad"], scene["pt_obs"], scene["kf_bad"], scene["conn"], scene["parent"], frame.get("prev") or [])
    out = dict(kf=kf)
    for name, cur, table, bad, nobs in (("points", held, scene["held"], scene["pt_bad"], scene["pt_nobs"]),
                                        ("lines", lheld, scene["lheld"], scene["ln_bad"], scene["ln_nobs"])):
        local = update_local_elements(kf["local_kf"], table, bad)
        seen = search_first_loop(cur, bad)
        out[name] = dict(local=local, flags=element_flags(local, seen, nobs), cur_flags=held_flags(cur, nobs))
    return out


def first_occurrence_scan(local_kf, kf_held, bad):
    """mvpLocalMapPoints by brute force: every (list position, slot) pair in order, kept when no earlier pair names the same live element."""
    pairs = [(pos, i, p) for pos, kf in enumerate(local_kf) for i, p in enumerate(kf_held[kf]) if p is not None and not bad[p]]
    return [p for n, (pos, i, p) in enumerate(pairs) if all(q != p for _, _, q in pairs[:n])]
