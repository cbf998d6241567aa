"""A literal Python restatement of the covisibility walks of the reference, independent of the library:
KeyFrame::UpdateConnections (src/KeyFrame.cpp:629-711) and the loop of LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:802-862)
with what KeyFrame::SetBadFlag (src/KeyFrame.cpp:936-995) does to the map points between two keyframes of that loop.

The map is built from the same records the index stores (per keyframe and feature: a table slot and an octave), under the
invariant the reference keeps on the server:  pMP->mObservations contains (pKF, idx)  iff  pKF->mvpMapPoints[idx] == pMP.
A keyframe that holds one point at two features cannot be written down in a std::map<kfptr, size_t>; RefMap refuses it."""
import numpy as np

NO_SLOT = 2 ** 31 - 1


class RefMap:
    def __init__(self, records, flags=None, rank=None):
        """records: key -> (slot per feature, octave per feature).  flags: the map-point table's flags column (uint8 per slot,
        1 = LIVE, 2 = BAD) or None: no point is bad.  rank: key -> position in the iteration of a std::map<kfptr, ...> (pointer
        order); None: ascending key."""
        self.mp = {}            # key -> mvpMapPoints: point id or None per feature
        self.octave = {}        # key -> mvKeysUn[i].octave
        self.kf_bad = set()
        self.obs = {}           # point id -> {key: feature index}   (mObservations)
        self.mp_bad = set()
        self.rank = dict(rank) if rank is not None else {k: i for i, k in enumerate(sorted(records))}
        for key, (slot, octave) in records.items():
            ids = []
            for i, s in enumerate(np.asarray(slot).tolist()):
                if s < 0 or s == NO_SLOT:                              # NO_SLOT: the index's "a point without a table slot yet".  It
                    ids.append(None)                                   # holds no point by the index's definition; the caller walks
                    continue                                           # the map itself for a keyframe with such a feature
                pid = int(s)
                if key in self.obs.setdefault(pid, {}):
                    raise ValueError("keyframe %r holds point %r twice: not a state of the reference" % (key, pid))
                self.obs[pid][key] = i
                ids.append(pid)
                if flags is not None and (pid >= len(flags) or (int(flags[pid]) & 3) != 1):
                    self.mp_bad.add(pid)
            self.mp[key] = ids
            self.octave[key] = [int(o) for o in np.asarray(octave).tolist()]

    # ---- what the walks read
    def _observations(self, pid):
        """GetObservations(): a copy, iterated in pointer order"""
        return sorted(self.obs.get(pid, {}).items(), key=lambda kv: self.rank[kv[0]])

    def Observations(self, pid):
        return len(self.obs.get(pid, {}))

    # ---- KeyFrame::UpdateConnections, :629-711
    def update_connections(self, key, th=15):
        """Returns (KFcounter as {key: weight}, mvpOrderedConnectedKeyFrames, mvOrderedWeights); the two lists are None when the
        function returns early (:664) and leaves the connections as they are."""
        counter = {}
        for pid in self.mp[key]:                                        # :644
            if pid is None:
                continue
            if pid in self.mp_bad:                                      # :651
                continue
            for kf, _ in self._observations(pid):                       # :656
                if kf == key:
                    continue
                counter[kf] = counter.get(kf, 0) + 1
        if not counter:                                                 # :664
            return counter, None, None
        nmax, kfmax = 0, None
        pairs = []
        for kf in sorted(counter, key=lambda k: self.rank[k]):          # :677, a std::map<kfptr, int>
            w = counter[kf]
            if w > nmax:                                                # :679
                nmax, kfmax = w, kf
            if w >= th:                                                 # :684
                pairs.append((w, kf))
        if not pairs:                                                   # :691
            pairs.append((nmax, kfmax))
        pairs.sort(key=lambda p: (p[0], self.rank[p[1]]))               # :697, pair<int, kfptr>
        kfs, ws = [], []
        for w, kf in pairs:                                             # :700, push_front
            kfs.insert(0, kf); ws.insert(0, w)
        return counter, kfs, ws

    # ---- KeyFrame::SetBadFlag, :936-995, as far as it touches what the walks read
    def set_bad_flag(self, key):
        """Returns the points that turned bad."""
        turned = []
        if key in self.kf_bad:
            return turned
        for i, pid in enumerate(self.mp[key]):                          # :990
            if pid is None:
                continue
            turned += self._erase_observation(pid, key)
        self.kf_bad.add(key)
        return turned

    def _erase_observation(self, pid, key):                             # MapPoint::EraseObservation, src/MapPoint.cpp:442-510
        obs = self.obs.get(pid, {})
        if key not in obs:
            return []
        del obs[key]
        if len(obs) <= 2 and pid not in self.mp_bad:                    # :494 "If only 2 observations or less, discard point"
            self.mp_bad.add(pid)                                        # MapPoint::SetBadFlag, :523-558
            for kf, idx in list(obs.items()):
                self.mp[kf][idx] = None                                 # EraseMapPointMatch
            obs.clear()
            return [pid]
        return []

    # ---- LocalMapping::KeyFrameCullingV3, the loop :802-862
    def counts(self, key, th_obs=3):
        """(nMPs, nRedundantObservations) of one keyframe, :815-855"""
        n_redundant, n_mps = 0, 0
        for i, pid in enumerate(self.mp[key]):                          # :818
            if pid is None:
                continue
            if pid in self.mp_bad:                                      # :823
                continue
            n_mps += 1
            if self.Observations(pid) > th_obs:                         # :826
                level = self.octave[key][i]
                n_obs = 0
                for kfi, idx in self._observations(pid):                # :831
                    if kfi in self.kf_bad:                              # :835
                        continue
                    if kfi == key:
                        continue
                    if self.octave[kfi][idx] <= level + 1:              # :841
                        n_obs += 1
                        if n_obs >= th_obs:
                            break
                if n_obs >= th_obs:
                    n_redundant += 1
        return n_mps, n_redundant

    def keyframe_culling(self, local_keys, protected_keys, thres, th_obs=3):
        """Returns (culled keys in order, [(key, nMPs, nRedundantObservations)] per keyframe the loop looked at)."""
        culled, log = [], []
        for key in local_keys:                                          # :804
            if key in protected_keys:                                   # :807, :810
                continue
            n_mps, n_redundant = self.counts(key, th_obs)
            log.append((key, n_mps, n_redundant))
            if n_redundant > thres * n_mps:                             # :857, in double
                self.set_bad_flag(key)
                culled.append(key)
        return culled, log

    # ---- the records as the map holds them now (after set_bad_flag): what the caller puts into the index again
    def record(self, key):
        slot = [-1 if p is None else p for p in self.mp[key]]
        return np.array(slot, "i4"), np.array(self.octave[key], np.uint8)


def pair_weights(records, query_key, counts=None):
    """weights by the header's definition, for records the reference cannot hold (a point twice in a keyframe): per stored key the
    number of pairs (counting entry of the query, entry of the record) with equal slots.  counts(slot) -> bool."""
    q = [int(s) for s in np.asarray(records[query_key][0]).tolist() if 0 <= s < NO_SLOT and (counts is None or counts(int(s)))]
    out = {}
    for key, (slot, _) in records.items():
        if key == query_key:
            continue
        other = [int(s) for s in np.asarray(slot).tolist() if 0 <= s < NO_SLOT]
        out[key] = sum(1 for a in q for b in other if a == b)
    return out
