"""KeyFrameDatabase reference for the tests: a literal transcription of the inverted-file walk of cslam's Database.cpp.

`RefDatabase` keeps `mvInvertedFile` (a list of keyframes per word) and the per-keyframe fields the walk writes (`mnLoopWords`,
`mLoopQuery` / `mMatchQuery`, `mLoopScore`), and runs DetectLoopCandidates / DetectMapMatchCandidates statement by statement.  It
knows nothing of slots, sequence numbers or a `(first_word, seq)` order: the library's formulation and this one check each other.
Scores are a plain Python loop over the two vectors (L1Scoring::score).  Floats are numpy float32 where the reference's are float."""
import numpy as np

F = np.float32


def l1_score(ids1, vals1, ids2, vals2, order=None):
    """L1Scoring::score (ScoringObject.cpp:23-68): the merge walk, one double, terms added as the walk meets them.
    order: None = the walk's order; "reversed" / "tree" add the same terms in another order (the GPU test shows that it matters)."""
    terms = []
    a = b = 0
    n1, n2 = len(ids1), len(ids2)
    while a < n1 and b < n2:
        if ids1[a] == ids2[b]:
            vi, wi = float(vals1[a]), float(vals2[b])
            terms.append(abs(vi - wi) - abs(vi) - abs(wi))
            a += 1; b += 1
        elif ids1[a] < ids2[b]:
            a += 1
        else:
            b += 1
    if order == "reversed":
        terms = terms[::-1]
    if order == "tree":
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    score = 0.0
    for t in terms:
        score += t
    return -score / 2.0


def per_entry(q_ids, q_vals, e_ids, e_vals):
    """(words, first_word, score) of one entry for one query: what the device computes per slot."""
    common = np.intersect1d(np.asarray(q_ids, "i8"), np.asarray(e_ids, "i8"))
    if len(common) == 0:
        return 0, -1, 0.0
    return len(common), int(common[0]), l1_score(q_ids, q_vals, e_ids, e_vals)


class KF:
    """The fields of cslam::KeyFrame the database touches."""

    def __init__(self, key, ids, vals, map_id=0, client=0):
        self.key, self.map_id, self.client = key, map_id, client
        self.ids = [int(i) for i in ids]; self.vals = [float(v) for v in vals]      # mBowVec, in key order
        self.connected = set()            # GetConnectedKeyFrames(): keys
        self.best_covis = []              # GetBestCovisibilityKeyFrames(10): KF objects, best first
        self.mnLoopWords = 0; self.mLoopQuery = None; self.mMatchQuery = None; self.mLoopScore = F(0)


class RefDatabase:
    def __init__(self):
        self.inverted = {}                # mvInvertedFile: word -> list of KF (a dict: only the touched words exist)

    def add(self, kf):                    # :37-43
        for w in kf.ids:
            self.inverted.setdefault(w, []).append(kf)

    def erase(self, kf):                  # :45-64
        for w in kf.ids:
            lst = self.inverted.get(w, [])
            for i, other in enumerate(lst):
                if other is kf:
                    del lst[i]
                    break

    def clear(self):                      # :66-70
        self.inverted = {}

    def _finish(self, kf, min_score, sharing, query_field):
        out = {"listed": [k.key for k in sharing], "min_common_words": 0, "shortlist": [], "candidates": []}
        if not sharing:                                                          # :111
            return out
        max_common = 0
        for k in sharing:                                                        # :117-122
            if k.mnLoopWords > max_common:
                max_common = k.mnLoopWords
        min_common = int(F(max_common) * F(0.8))                                 # :124  int minCommonWords = maxCommonWords*0.8f
        score_and_match = []
        for k in sharing:                                                        # :129-143
            if k.mnLoopWords > min_common:
                si = F(l1_score(kf.ids, kf.vals, k.ids, k.vals))
                k.mLoopScore = si
                if si >= F(min_score):
                    score_and_match.append((si, k))
        if not score_and_match:                                                  # :145
            return out
        out["min_common_words"] = min_common
        out["shortlist"] = [k.key for _, k in score_and_match]
        acc_and_match = []
        best_acc = F(min_score)                                                  # :149
        for si, k in score_and_match:                                            # :152-178
            best, acc, best_kf = si, si, k
            for k2 in k.best_covis[:10]:
                if getattr(k2, query_field) == kf.key and k2.mnLoopWords > min_common:
                    acc = F(acc + k2.mLoopScore)
                    if k2.mLoopScore > best:
                        best_kf, best = k2, k2.mLoopScore
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = F(F(0.75) * best_acc)                                           # :181
        added = set()
        for acc, k in acc_and_match:                                             # :187-198
            if acc > retain and k.key not in added:
                out["candidates"].append(k.key)
                added.add(k.key)
        return out

    def detect_loop(self, kf, min_score, keys_in_map):
        """DetectLoopCandidates (:72-202); keys_in_map = the keys of pKF->GetMapptr()->GetMmpKeyFrames()."""
        sharing = []
        for w in kf.ids:                                                         # :84-108
            for k in self.inverted.get(w, []):
                if k.key == kf.key:
                    continue
                if k.key not in keys_in_map:
                    continue
                if k.mLoopQuery != kf.key:
                    k.mnLoopWords = 0
                    if k.key not in kf.connected:
                        k.mLoopQuery = kf.key
                        sharing.append(k)
                k.mnLoopWords += 1
        return self._finish(kf, min_score, sharing, "mLoopQuery")

    def detect_map_match(self, kf, min_score, ass_clients):
        """DetectMapMatchCandidates (:204-327); ass_clients = pMap->msuAssClients."""
        sharing = []
        for w in kf.ids:                                                         # :213-233
            for k in self.inverted.get(w, []):
                if k.mMatchQuery != kf.key:
                    k.mnLoopWords = 0
                    if k.client not in ass_clients:
                        k.mMatchQuery = kf.key
                        sharing.append(k)
                k.mnLoopWords += 1
        return self._finish(kf, min_score, sharing, "mMatchQuery")


def min_score(kf, connected_kfs):
    """LoopFinder.cpp:122-139 / MapMatcher.cpp:130-147 (the caller leaves out the bad keyframes)."""
    m = F(1)
    for k in connected_kfs:
        s = F(l1_score(kf.ids, kf.vals, k.ids, k.vals))
        if s < m:
            m = s
    return m


def random_bow(rng, n, n_words, scales=(1.0,)):
    """A BowVector of n distinct words below n_words, L1-normalised; values uniform, each scaled by a factor drawn from `scales`."""
    ids = np.sort(rng.choice(n_words, size=n, replace=False)).astype("i4")
    v = rng.uniform(0.05, 1.0, n) * rng.choice(np.asarray(scales, "f8"), n)
    if n:
        v = v / np.abs(v).sum()
    return ids, v.astype("f8")
