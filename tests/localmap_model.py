"""Model of Tracking::UpdateLocalMap (reference src/Tracking.cc:1794-1949) in plain Python / NumPy, written from the reference's
loops: the keyframe votes (:1838-1855), K1 (:1871-1886), the K2 walk with its outer `break` (:1892-1942) and the point list
(:1794-1824).  Objects are slots: a keyframe's or point's slot number stands for its pointer, so "pointer order" is slot order."""
import numpy as np

BAD = 1


def observations_of(obs):
    """point slot -> the keyframes of its live records (a std::map<KeyFrame*, size_t>: ascending, each keyframe once)."""
    out = {}
    for p, k in zip(obs["point"].tolist(), obs["keyframe"].tolist()):
        if p >= 0:
            out.setdefault(p, set()).add(k)
    return {p: sorted(ks) for p, ks in out.items()}


def votes(obs, point_flags, frame_points, n_kfs):
    """keyframeCounter (:1836-1855) as an array over the keyframe slots (0 = not in the map)."""
    seen_by = observations_of(obs)
    counter = np.zeros(n_kfs, np.int32)
    for p in np.asarray(frame_points).tolist():
        if p < 0:
            continue                                   # mvpMapPoints[i] == NULL
        if point_flags[p] & BAD:
            continue                                   # (:1852 nulls the entry)
        for k in seen_by.get(p, ()):
            counter[k] += 1
    return counter


def local_keyframes(counter, kf_bad, neighbours, children, parent, marks, frame_id, outer_break=True):
    """:1857-1948.  counter: votes per keyframe slot; neighbours[k]: GetBestCovisibilityKeyFrames(10) of k, in its order; children[k]:
    GetChilds() in set (slot) order; parent[k]: slot or -1; marks: mnTrackReferenceForFrame per keyframe, written as the reference
    writes it.  -> (local keyframes in order, reference keyframe or -1), or None where :1857 returns early.
    outer_break=False is the walk as it would be if the parent branch's break left nothing (what the test shows to differ)."""
    voted = [k for k in range(len(counter)) if counter[k] > 0]
    if not voted:
        return None
    best, ref, local = 0, -1, []
    for k in voted:                                    # std::map order = ascending pointer
        if kf_bad[k]:
            continue
        if counter[k] > best:
            best, ref = int(counter[k]), k
        local.append(k); marks[k] = frame_id
    for k in list(local):                              # (the end iterator is taken before the walk: K1 only)
        if len(local) > 80:
            break
        for nb in neighbours[k][:10]:
            if not kf_bad[nb] and marks[nb] != frame_id:
                local.append(nb); marks[nb] = frame_id
                break
        for ch in sorted(children[k]):
            if not kf_bad[ch] and marks[ch] != frame_id:
                local.append(ch); marks[ch] = frame_id
                break
        pa = parent[k]
        if pa >= 0 and marks[pa] != frame_id:
            local.append(pa); marks[pa] = frame_id
            if outer_break:
                break                                  # :1938 leaves the OUTER loop
    return local, ref


def local_points(kf_rows, kf_count, point_flags, local_kfs):
    """:1794-1824 over the rows of the listed keyframes; every call starts unmarked."""
    marked, out = set(), []
    for k in np.asarray(local_kfs).tolist():
        for s in kf_rows[k, :kf_count[k]].tolist():
            if s < 0 or s in marked:
                continue
            if point_flags[s] & BAD:
                continue
            out.append(s); marked.add(s)
    return np.array(out, np.int32)
