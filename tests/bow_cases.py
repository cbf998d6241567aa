"""Hand-built cases for tests/bow_ref.py (the definition), the CPU oracle and the kernels that walk the vocabulary tree or a
FeatureVector.  Every descriptor is a set of bit positions, so the Hamming distance of two of them is the size of the symmetric
difference of their sets and every distance below is known by construction; each builder's docstring derives the expected answer,
which tests/test_bow_cases_cpu.py writes down (HAND) and holds the definition to.

A case is a dict: name, kind, args, forces (trace keys the case must reach, with the least count).  run_ref(case) is the definition's
answer; all_cases() lists every case.  Nothing here takes the workload's sizes: the largest frame side has 4097 features (the
directory's host / device threshold), the matcher cases at most 129."""
import itertools

import numpy as np

import bow_ref as R

F = np.float32


def D(*parts):
    """The descriptor with the bits of the half-open ranges `parts` set."""
    b = np.zeros(256, np.uint8)
    for lo, hi in parts:
        b[lo:hi] = 1
    return np.packbits(b)


ZERO, ONES = D(), D((0, 256))


def near(d):
    """A descriptor at distance d from ZERO."""
    return D((0, d))


# ------------------------------------------------------------------------------------------------------------ descent
# The logical tree of the descent cases (k = 2, real depth 2):
#   A = [0,8)   -> A1 = A + [100,104), A2 = A + [110,114)
#   B = [8,16)  -> B1 = B + [120,124), B2 = B + [130,134), B3 = B + [140,144)      three children, more than k
#   C = [16,24)    a leaf directly under the root
#   E = [24,32) -> E1 = E + [150,152)                                              a single-child chain
TREE = dict(A=("root", [(0, 8)], 0.0), A1=("A", [(0, 8), (100, 104)], 1.5), A2=("A", [(0, 8), (110, 114)], 0.0),
            B=("root", [(8, 16)], 0.0), B1=("B", [(8, 16), (120, 124)], -0.0), B2=("B", [(8, 16), (130, 134)], -2.0),
            B3=("B", [(8, 16), (140, 144)], 5e-324), C=("root", [(16, 24)], 2.25), E=("root", [(24, 32)], 0.0),
            E1=("E", [(24, 32), (150, 152)], 0.75))
ORDERS = dict(depth_first=["A", "A1", "A2", "B", "B1", "B2", "B3", "C", "E", "E1"],
              breadth_first=["A", "B", "C", "E", "A1", "A2", "B1", "B2", "B3", "E1"],
              interleaved=["A", "B", "A1", "C", "B1", "E", "A2", "B2", "E1", "B3"])
# feature -> (bits, the leaf it reaches, its level-1 node); distances per level:
#   f0 = A1         level 1: A 4, B C E 20 -> A;  level 2: A1 0, A2 8 -> A1                       (a distance of 0)
#   f1 = [0,8)      A 0 -> A;  A1 4, A2 4: the first of two equal children -> A1                  (tie at the last level)
#   f2 = nothing    A B C E all 8: the first of all -> A;  A1 12, A2 12 -> A1                     (tie of all children, first level)
#   f3 = [0,4)+[8,12)+[110,114)   A 12, B 12, C E 20: the first of two -> A;  A1 16, A2 8 -> A2   (tie of two, first level)
#   f4 = [8,16)     B 0 -> B;  B1 B2 B3 all 4 -> B1                                               (three children > k, all equal)
#   f5 = [16,24)    C 0 -> C, a leaf at level 1
#   f6 = [24,32)    E 0 -> E;  its only child E1
#   f7 = all ones   A B C E 248 -> A;  A1 A2 244 -> A1
#   f8 = B2, f9 = B3   B 4 -> B;  the leaf itself at 0, its siblings at 8
FEATS = [([(0, 8), (100, 104)], "A1", "A"), ([(0, 8)], "A1", "A"), ([], "A1", "A"), ([(0, 4), (8, 12), (110, 114)], "A2", "A"),
         ([(8, 16)], "B1", "B"), ([(16, 24)], "C", "C"), ([(24, 32)], "E1", "E"), ([(0, 256)], "A1", "A"),
         ([(8, 16), (130, 134)], "B2", "B"), ([(8, 16), (140, 144)], "B3", "B")]


def tree(order):
    """(parent, desc, weight, name -> node id) of TREE with its nodes in the given order."""
    names = ["root"] + ORDERS[order]
    ident = {n: i for i, n in enumerate(names)}
    parent = np.array([0] + [ident[TREE[n][0]] for n in names[1:]], np.int32)
    desc = np.stack([ZERO] + [D(*TREE[n][1]) for n in names[1:]])
    weight = np.array([0.0] + [TREE[n][2] for n in names[1:]], np.float64)
    return parent, desc, weight, ident


def descent(order, L=2, levelsups=None, n=None):
    """TREE in one node order, the ten features (tiled to n when given) at every levelsup of {0, L-1, L, L+2}.  The expected
    (word, weight, nid) per feature: word = the rank of the reached leaf among the leaves in NODE order, weight = that leaf's, nid =
    the node on the path at level L - levelsup, 0 when that level is <= 0 or below the leaf (C is at level 1; with L = 4 declared
    over the real depth 2 every leaf is above levels 3 and 4).  Then Frame::ComputeBoW's part: the FeatureVector node per feature
    (nid where the weight is > 0: A2 at 0.0, B1 at -0.0 and B2 at -2.0 drop out, B3 at 5e-324 stays) and the directory of those nodes.
    The tiled forms run at levelsup 0 and 1; 4096 and 4097 features sit on either side of the size at which a frame handle builds
    its directory on the device or on the host."""
    parent, desc, weight, _ = tree(order)
    feats = np.stack([D(*f[0]) for f in FEATS])
    if n is not None:
        feats = feats[np.arange(n) % len(FEATS)]
    lv = list(levelsups if levelsups is not None else (0, L - 1, L, L + 2))
    name = "descent_%s" % order + ("_L%d" % L if L != 2 else "") + ("_n%d" % n if n is not None else "")
    forces = dict(child_tie=1, child_tie_all=1, child_tie_level_1=1, child_tie_level_2=1, more_than_k_children=1, child_dist_0=1) if n != 1 else {}
    if 0 in lv and n != 1:
        forces["leaf_above_nid_level"] = 1
    return dict(name=name, kind="descent", forces=forces,
                args=dict(k=2, L=L, parent=parent, desc=desc, weight=weight, feats=feats, levelsups=lv))


def descent_extremes():
    """root -> X = nothing, Y = all ones, P = [0,128) -> T1 = T2 = [0,128) (identical siblings); k = 3, L = 2, depth first: X 1, Y 2, P 3,
    T1 4, T2 5; words X 0, Y 1, T1 2, T2 3.
      g0 = nothing   X 0, Y 256, P 128 -> X        g1 = all ones   X 256, Y 0 -> Y
      g2 = [0,128)   P 0 -> P; T1 0, T2 0 -> T1 (the first twin)
      g3 = [0,64)    X 64, Y 192, P 64: the first of X and P -> X"""
    parent = np.array([0, 0, 0, 0, 3, 3], np.int32)
    desc = np.stack([ZERO, ZERO, ONES, D((0, 128)), D((0, 128)), D((0, 128))])
    weight = np.array([0.0, 1.0, 2.0, 0.0, 3.0, 4.0])
    feats = np.stack([ZERO, ONES, D((0, 128)), D((0, 64))])
    return dict(name="descent_extremes", kind="descent", forces=dict(child_dist_0=1, child_dist_256=1, child_tie=2),
                args=dict(k=3, L=2, parent=parent, desc=desc, weight=weight, feats=feats, levelsups=[0, 1, 2, 4]))


# ------------------------------------------------------------------------------------------------------------ BowVector, score
COMBOS = list(itertools.product((R.TF_IDF, R.TF, R.IDF, R.BINARY), (R.L1_NORM, R.L2_NORM, R.DOT_PRODUCT)))


def bowvec_weights():
    """The ten features of descent_depth_first at levelsup 1: words A1 A1 A1 A2 B1 C E1 A1 B2 B3 = 0 0 0 1 2 5 6 0 3 4 with weights
    1.5 1.5 1.5 0.0 -0.0 2.25 0.75 1.5 -2.0 5e-324 and level-1 nodes A A A A B C E A B B = 1 1 1 1 4 8 9 1 4 4.  Only w > 0 counts: 0.0, -0.0
    and -2.0 are stopped, the smallest denormal is not.  Kept: word 0 four times, words 4, 5, 6 once; fv = 1 1 1 -1 -1 8 9 1 -1 4."""
    return dict(name="bowvec_weights", kind="bowvec", forces=dict(stopped=3),
                args=dict(word_id=np.array([0, 0, 0, 1, 2, 5, 6, 0, 3, 4], np.int32),
                          weight=np.array([1.5, 1.5, 1.5, 0.0, -0.0, 2.25, 0.75, 1.5, -2.0, 5e-324]),
                          node_id=np.array([1, 1, 1, 1, 4, 8, 9, 1, 4, 4], np.int32)))


def bowvec_many_hits():
    """Word 7 hit 1200 times with 0.1 (600, then word 3 once with 2.0, then 600), word 9 three times with 0.3.  addWeight adds in
    feature order: the value of word 7 is 0.1 added 1199 times to 0.1 (119.99999999999746), not the pairwise sum (120.0)."""
    wid = np.array([7] * 600 + [3] + [7] * 600 + [9] * 3, np.int32)
    w = np.where(wid == 7, 0.1, np.where(wid == 3, 2.0, 0.3))
    return dict(name="bowvec_many_hits", kind="bowvec", forces=dict(max_hits=1200),
                args=dict(word_id=wid, weight=w, node_id=(np.arange(len(wid)) % 5).astype(np.int32)))


def bowvec_all_stopped():
    """Every weight is 0.0, -0.0 or negative: no word, every fv node -1."""
    w = np.array([0.0, -0.0, -1.0] * 3)
    return dict(name="bowvec_all_stopped", kind="bowvec", forces=dict(stopped=9),
                args=dict(word_id=np.arange(9, dtype=np.int32), weight=w, node_id=np.arange(9, dtype=np.int32) + 3))


def scores():
    """L1 score pairs: disjoint ids -> -0 / 2 = 0; identical [0.5, 0.5] -> each word gives |0| - 0.5 - 0.5 = -1, score 1; nested ({2} in
    {1, 2, 3}: |0.25 - 1| - 0.25 - 1 = -0.5 -> 0.25); an empty vector on either side -> 0; ids that leapfrog (1 4 6 9 against 2 4 5 9:
    common 4 and 9)."""
    a = (np.array([1, 3], np.int32), np.array([0.5, 0.5]))
    b = (np.array([2, 4], np.int32), np.array([0.25, 0.75]))
    n3 = (np.array([1, 2, 3], np.int32), np.array([0.5, 0.25, 0.25]))
    n1 = (np.array([2], np.int32), np.array([1.0]))
    e = (np.zeros(0, np.int32), np.zeros(0))
    p = (np.array([1, 4, 6, 9], np.int32), np.array([0.125, 0.25, 0.5, 0.125]))
    q = (np.array([2, 4, 5, 9], np.int32), np.array([0.25, 0.5, 0.125, 0.125]))
    return dict(name="scores", kind="score", forces={}, args=dict(pairs=[(a, b), (a, a), (n1, n3), (n3, n1), (e, a), (a, e), (e, e), (p, q)]))


# ------------------------------------------------------------------------------------------------------------ distinctive
def _rows(n, zero_rows):
    """n rows: the rows of zero_rows are ZERO, every other row r has the single bit r.  Two different single-bit rows are 2 apart, a
    single-bit row and a ZERO row 1, equal rows 0.  With z ZERO rows and m = int(0.5 * (n - 1)): a ZERO row's sorted distances are z
    zeros then ones, its median 0 if m < z else 1; a single-bit row's are one 0, z ones, then twos: 0 if m = 0, 1 if m <= z, else 2."""
    d = np.zeros((n, 32), np.uint8)
    for r in range(n):
        if r not in zero_rows:
            d[r] = D((r, r + 1))
    return d


def distinctive_groups():
    """name -> rows; the expected row per group (m = int(0.5 * (N - 1)), z = number of ZERO rows, see _rows):
      n0    no row: -1 (the project's answer; the reference returns early)          n1    one row: 0
      n2    m = 0: every median is the row's own 0, the first row: 0
      n3    ZERO rows 1, 2: m = 1 < z: they have 0, row 0 has 1 -> 1, the first of the two equal
      n4    ZERO rows 2, 3: m = 1 < z = 2 -> 0 against 1 -> 2.  Read at N / 2 = 2 = z every row has 1 and row 0 would win
      n63   ZERO rows 61, 62: m = 31 > z: 1 against 2 -> 61
      n64   ZERO rows 32..63: m = 31 < z = 32 -> 32.  Read at N / 2 = 32 every row has 1 -> row 0
      n65   ZERO rows 63, 64: m = 32: 1 against 2 -> 63; row 64 is equal and sits in lane 0 of the second round
      n128  ZERO rows 64..127: m = 63 < z = 64 -> 64
      n129  ZERO rows 127, 128: m = 64: 1 against 2 -> 127; row 128 is equal, lane 0 of the third round
      same  five identical rows: all medians 0 -> 0
      compl b, ~b, ~b: row 0 has 0 256 256 -> median 256; rows 1 and 2 have 0 0 256 -> 0 -> 1"""
    b = D((3, 77), (100, 130))
    return dict(n0=np.zeros((0, 32), np.uint8), n1=_rows(1, ()), n2=_rows(2, (1,)), n3=_rows(3, (1, 2)), n4=_rows(4, (2, 3)),
                n63=_rows(63, (61, 62)), n64=_rows(64, range(32, 64)), n65=_rows(65, (63, 64)), n128=_rows(128, range(64, 128)),
                n129=_rows(129, (127, 128)), same=np.tile(b, (5, 1)), compl=np.stack([b, ~b, ~b]))


def distinctive_calls():
    """Calls of 1, 3, 4, 5 and all 12 map points.  The library takes one descriptor pool with (first, count) per point; the pool is laid
    out in REVERSE order of the points, so `first` descends."""
    g = distinctive_groups()
    calls = [["n65"], ["n3", "n0", "n129"], ["n4", "n64", "n1", "compl"], ["n2", "n63", "same", "n128", "n65"], list(g)]
    return [dict(name="distinctive_%d" % len(c), kind="distinctive", args=dict(groups=[g[k] for k in c], names=c),
                 forces=dict(median_tie=1, median_tie_later_row_smaller_lane=1) if "n65" in c or "n129" in c else {}) for c in calls]


def pool(groups):
    """(desc, first, count) with the groups stored last to first."""
    first = np.zeros(len(groups), np.int64)
    at = 0
    parts = []
    for p in reversed(range(len(groups))):
        first[p] = at
        at += len(groups[p])
        parts.append(groups[p])
    desc = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(desc), first, np.array([len(x) for x in groups], np.int32)


# ------------------------------------------------------------------------------------------------------------ directory
DIR_SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097)
BIG = (1 << 30) - 1
HANDLE_BIG = (1 << 24) - 1


def directory_patterns(n):
    """name -> node per feature, for n features:
      one_node   every feature in node 0: order 0..n-1, nodes [0], first [0, n]
      distinct   node BIG - i (ids near 2^30, descending): order n-1..0, nodes BIG-n+1..BIG, first 0..n
      distinct24 the same below HANDLE_BIG = 2^24 - 1, the largest node id a frame handle takes (ccm_frame_set_bow refuses 2^24 and above)
      stopped    every node -1: all three empty but first = [0]
      mixed      node i % 3 - 1 (a third without a node): node 0 holds i = 1, 4, 7, .., node 1 holds i = 2, 5, 8, .."""
    i = np.arange(n)
    return dict(one_node=np.zeros(n, np.int32), distinct=(BIG - i).astype(np.int32), distinct24=(HANDLE_BIG - i).astype(np.int32),
                stopped=np.full(n, -1, np.int32), mixed=(i % 3 - 1).astype(np.int32))


def directory_cases():
    out = [dict(name="directory_%d" % n, kind="directory", forces={}, args=dict(patterns=directory_patterns(n))) for n in DIR_SIZES]
    out.append(dict(name="directory_small", kind="directory", forces={},
                    args=dict(patterns=dict(hand=np.array([7, -1, 7, 0, BIG], np.int32),          # order 3 0 2 4, nodes 0 7 BIG, first 0 1 3 4
                                            hand24=np.array([9, HANDLE_BIG, -1, 9, 2, -1, 9], np.int32)))))   # order 4 0 3 6 1, nodes 2 9 HANDLE_BIG, first 0 1 4 5
    return out


GRID = 65


def _code(a, at):
    return [(at + j, at + j + 1) for j in range(7) if (a >> j) & 1]


def grid_vocabulary():
    """root -> 65 nodes a -> 65 leaves (a, b) each, depth first: node a = 1 + 66 a, leaf (a, b) = 2 + 66 a + b, word = 65 a + b.  Node a
    carries the binary code of a in bits [0,7), leaf (a, b) that and the code of b in bits [8,15).  The feature (a, b) IS the leaf's
    descriptor: at level 1 node a' is at popcount(a ^ a') + popcount(b), least at a' = a alone; at level 2 leaf b' is at
    popcount(b ^ b'), 0 at b' = b alone.  The leaves of a = 64 have weight 0 (stopped), every other 1 + word / 8192."""
    parent, desc, weight = [0], [ZERO], [0.0]
    for a in range(GRID):
        parent.append(0); desc.append(D(*_code(a, 0))); weight.append(0.0)
        for b in range(GRID):
            parent.append(1 + 66 * a); desc.append(D(*(_code(a, 0) + _code(b, 8)))); weight.append(0.0 if a == 64 else 1.0 + (65 * a + b) / 8192.0)
    return dict(k=GRID, L=2, parent=np.array(parent, np.int32), desc=np.stack(desc), weight=np.array(weight))


def grid_pairs(pattern, n):
    """(a, b) per feature: distinct = leaf i (a = i // 65, b = i % 65; the last 65 of 4225 are stopped, n stays below); one_node = a = 3
    for all; stopped = a = 64 for all; mixed = a = (7 i) % 20, but 64 (stopped) for every 13th feature, b = (11 i) % 65: about n / 20
    features per node."""
    i = np.arange(n)
    if pattern == "distinct":
        return i // GRID, i % GRID
    if pattern == "one_node":
        return np.full(n, 3), i % GRID
    if pattern == "stopped":
        return np.full(n, 64), i % GRID
    return np.where(i % 13 == 0, 64, (7 * i) % 20), (11 * i) % GRID


def grid_case(pattern, n, levelsup):
    a, b = grid_pairs(pattern, n)
    voc = grid_vocabulary()
    feats = voc["desc"][2 + 66 * a + b] if n else np.zeros((0, 32), np.uint8)
    return dict(name="grid_%s_%d_up%d" % (pattern, n, levelsup), kind="grid", forces={}, pairs=(a, b),
                args=dict(voc=voc, feats=np.ascontiguousarray(feats), levelsup=levelsup))


def grid_cases():
    """distinct at levelsup 0 (every feature its own node) and mixed at levelsup 1 (about n / 20 features per node, a stopped share) at
    every size; one node at levelsup 1, node 0 for everything (levelsup 2) and all stopped at the small sizes and at 1025 and 4097."""
    out = []
    for n in DIR_SIZES:
        out += [grid_case("distinct", n, 0), grid_case("mixed", n, 1)]
        if n <= 5 or n in (1025, 4097):
            out += [grid_case("one_node", n, 1), grid_case("mixed", n, 2), grid_case("stopped", n, 1)]
    return out


# ------------------------------------------------------------------------------------------------------------ SearchByBoW
def bow_case(name, groups, nnratio=0.6, check_ori=False, kfkf=False, loose1=(), loose2=(), forces=None):
    """groups: [(node, queries, candidates)], a query = (desc, valid1, angle), a candidate = (desc, valid2, angle); loose1 / loose2:
    (desc, node) features outside the groups.  Side 1 holds the queries group after group, side 2 the candidates."""
    s1, s2 = [], []
    for node, qs, cs in groups:
        s1 += [(q[0], node, q[1], q[2]) for q in qs]
        s2 += [(c[0], node, c[1], c[2]) for c in cs]
    s1 += [(d, nd, 1, 0.0) for d, nd in loose1]
    s2 += [(d, nd, 1, 0.0) for d, nd in loose2]

    def cols(s):
        if not s:
            return np.zeros((0, 32), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, F)
        return (np.stack([x[0] for x in s]), np.array([x[1] for x in s], np.int32), np.array([x[2] for x in s], np.uint8),
                np.array([x[3] for x in s], F))
    d1, n1, v1, a1 = cols(s1)
    d2, n2, v2, a2 = cols(s2)
    return dict(name=name + ("_kfkf" if kfkf else ""), kind="bow", forces=dict(forces or {}),
                args=dict(desc1=d1, node1=n1, valid1=v1, angle1=a1, desc2=d2, node2=n2, angle2=a2, valid2=v2 if kfkf else None, nnratio=nnratio,
                          check_ori=check_ori, kfkf=kfkf))


def _q(valid=1, angle=0.0, desc=ZERO):
    return (desc, valid, angle)


def _c(d, valid=1, angle=0.0):
    return (d if isinstance(d, np.ndarray) else near(d), valid, angle)


def _sized(size, special, filler=100):
    """One ZERO query against `size` candidates: those of `special` {position: distance}, every other at `filler`."""
    return [(4, [_q()], [_c(special.get(p, filler)) for p in range(size)])]


def bow_size_cases(kfkf):
    """One query, one node, side-2 groups of 1, 63, 64, 65, 128 and 129 (64 lanes per chunk), fillers at 100, nnratio 0.6:
      size_1            a lone candidate at 10: second stays 256, 10 < 153.6 -> 0
      size_63           10 at position 62, 20 at 0: 10 < 12 -> 62
      size_64           10 at position 63 (the last lane of the first chunk), second 100 -> 63
      size_65           10 at position 64 (lane 0 of the second chunk) -> 64
      size_128_dup      10 at positions 5 and 70: the second 10 is not < best, but < second: second = 10 = best, 10 < 6 fails -> -1
      size_129_tie      the same at positions 3 and 128 with nnratio 1.5: 10 < 15 holds and the FIRST of the two -> 3
      size_128_same     10 at 10, 16 at 20 (same chunk): 10 < 9.6 fails -> -1
      size_128_other    10 at 100, 16 at 10 (the second in the EARLIER chunk) -> -1
      size_129_last     10 at 10, 16 at 128 (the second alone in the third chunk) -> -1
      size_128_accept   10 at 100, 17 at 10: 10 < 10.2 -> 100"""
    mk = lambda name, size, special, forces, nn=0.6: bow_case("bow_" + name, _sized(size, special), nnratio=nn, kfkf=kfkf, forces=forces)
    return [mk("size_1", 1, {0: 10}, dict(lone_candidate=1, groups=1)),
            mk("size_63", 63, {62: 10, 0: 20}, dict(max_group2=63)),
            mk("size_64", 64, {63: 10}, dict(best_at_lane_63=1)),
            mk("size_65", 65, {64: 10}, dict(best_at_lane_0_of_a_later_chunk=1)),
            mk("size_128_dup", 128, {5: 10, 70: 10}, dict(second_eq_best=1, later_chunk_equals_best=1, ratio_rejected=1)),
            mk("size_129_tie", 129, {3: 10, 128: 10}, dict(best_tie=1, later_chunk_equals_best=1, max_group2=129), nn=1.5),
            mk("size_128_same", 128, {10: 10, 20: 16}, dict(second_in_same_chunk=1, ratio_rejected=1)),
            mk("size_128_other", 128, {100: 10, 10: 16}, dict(second_in_other_chunk=1, ratio_rejected=1)),
            mk("size_129_last", 129, {10: 10, 128: 16}, dict(second_in_other_chunk=1, ratio_rejected=1)),
            mk("size_128_accept", 128, {100: 10, 10: 17}, dict(second_in_other_chunk=1))]


def bow_taken(kfkf):
    """Two nodes, two queries each; side 2 = [c1, c0 | c3, c2].
    Node 5: c0 = [0,10), c1 = [10,40); q0 = nothing: c1 30, c0 10 -> 10 < 18, takes c0 (index 1).  q1 = [0,8): c0 at 2, c1 at 38; c0 is
      taken, so best = c1 at 38 with second 256 -> index 0.  (Untaken, q1 would choose c0; with c0 counted as second, 38 < 1.2 fails.)
    Node 9: c2 = [0,10), c3 = [10,40); q2 = nothing takes c2 (index 3).  q3 = [0,6)+[10,30): c3 at 26 + 30 - 40 = 16, c2 at 26 + 10 - 12 = 24;
      c2 is taken: best 16, second 256 -> c3 (index 2).  (With c2 as second: 16 < 14.4 fails.)
    match12 = 1 0 3 2; each frame feature back to its query: 1 0 3 2."""
    c0, c1 = D((0, 10)), D((10, 40))
    g5 = (5, [_q(), _q(desc=D((0, 8)))], [_c(c1), _c(c0)])
    g9 = (9, [_q(), _q(desc=D((0, 6), (10, 30)))], [_c(c1), _c(c0)])
    return bow_case("bow_taken", [g5, g9], kfkf=kfkf, forces=dict(skipped_taken=2, lone_candidate=2, groups=2))


def bow_valid(kfkf):
    """Three nodes; side 2 = [5, 40 | 5*, 20, 40 | 10, 12*, 40] (* = no good map point: valid2 = 0, read by the KeyFrame form only).
    Node 1: qx has valid1 = 0 and is skipped although 5 is at hand; qy (valid) then takes it: 5 < 24 -> index 0.
    Node 2: KeyFrame form: 5* is skipped, best 20 (index 3), second 40, 20 < 24 -> 3.  Frame form: best 5 (index 2), second 20 -> 2.
    Node 3: KeyFrame form: 12* is skipped, best 10 (index 5), second 40 -> 5.  Frame form: second 12, 10 < 7.2 fails -> -1.
    match12: KeyFrame -1 0 3 5; Frame -1 0 2 -1 with match21 = 1 -1 2 -1 -1 -1 -1 -1."""
    g1 = (1, [_q(valid=0), _q()], [_c(5), _c(40)])
    g2 = (2, [_q()], [_c(5, valid=0), _c(20), _c(40)])
    g3 = (3, [_q()], [_c(10), _c(12, valid=0), _c(40)])
    forces = dict(skipped_invalid1=1, groups=3)
    if kfkf:
        forces["skipped_invalid2"] = 2
    return bow_case("bow_valid", [g1, g2, g3], kfkf=kfkf, forces=forces)


def bow_thresholds(kfkf):
    """Four nodes, one ZERO query each; side 2 = [50, 100 | 51, 100 | 256 | 256, 10] (256 = all ones).
    50 with second 100 passes the ratio (50 < 60): accepted by `<= TH_LOW` (Frame form, index 0), not by `< TH_LOW` (KeyFrame form).
    51: neither.  A lone candidate at 256 is never below the initial 256: no best at all.  256 then 10: best 10, second stays 256 -> 6.
    Frame 0 -1 -1 6; KeyFrame -1 -1 -1 6."""
    gs = [(1, [_q()], [_c(50), _c(100)]), (2, [_q()], [_c(51), _c(100)]), (3, [_q()], [_c(ONES)]), (4, [_q()], [_c(ONES), _c(10)])]
    return bow_case("bow_thresholds", gs, kfkf=kfkf, forces=dict(best_eq_th=1, best_eq_th_plus_1=1, no_candidate=1, dist_256_candidate=1, groups=4))


def bow_ratio(kfkf, which):
    """ratio_075: best 30, second 40, nnratio 0.75: 0.75f * 40 = 30 exactly, 30 < 30 fails -> -1.
    ratio_08: best 40, second 50, nnratio 0.8: 0.8f = 0.800000011920929; the float product rounds to 40.0 and 40 < 40 fails -> -1, while in
    double 40.00000059604645 > 40 would accept."""
    if which == "075":
        return bow_case("bow_ratio_075", [(1, [_q()], [_c(30), _c(40)])], nnratio=0.75, kfkf=kfkf, forces=dict(ratio_equal=1, ratio_rejected=1))
    return bow_case("bow_ratio_08", [(1, [_q()], [_c(40), _c(50)])], nnratio=0.8, kfkf=kfkf,
                    forces=dict(ratio_equal=1, ratio_float_differs_from_double=1, ratio_rejected=1))


def bow_nodes(kfkf):
    """Five common nodes (7, 12, 20, 30, 35), nodes on one side only (3 and 41 on side 1; 8 and 15 on side 2) and features without a
    node on both sides whose descriptors are equal (they would match at distance 0 if -1 were a node).
    side 1: i0 node 3, i1 node 7, i2 node -1, i3 node 12, i4 node 20, i5 node 30, i6 node 41, i7 node 35
    side 2: j0 node -1, j1 node 7 at 10, j2 node 12 at 12, j3 node 15, j4 node 20 at 14, j5 node 30 at 16, j6 node 8, j7 node 35 at 18
    Every common node holds one lone pair within 50 -> match12 = -1 1 -1 2 4 5 -1 7."""
    s1 = [(ZERO, 3), (ZERO, 7), (ZERO, -1), (ZERO, 12), (ZERO, 20), (ZERO, 30), (ZERO, 41), (ZERO, 35)]
    s2 = [(ZERO, -1), (near(10), 7), (near(12), 12), (near(1), 15), (near(14), 20), (near(16), 30), (near(1), 8), (near(18), 35)]
    return bow_case("bow_nodes", [], kfkf=kfkf, loose1=s1, loose2=s2, forces=dict(groups=5, nodes_one_side_only=4, negative_nodes_both_sides=1))


def _pairs(rots, kfkf, name, forces):
    """One lone pair (distance 5) per node; pair i has angle1 - angle2 = rots[i], given as (angle1, angle2)."""
    gs = [(i, [_q(angle=a1)], [_c(5, angle=a2)]) for i, (a1, a2) in enumerate(rots)]
    return bow_case(name, gs, check_ori=True, kfkf=kfkf, forces=forces)


def bow_hist_cases(kfkf):
    """Rotation histograms (bin = round(rot / 30), every pair matches first, then all bins but the three fullest are cleared):
      hist_ties        rot 0 0 30 30 60 60 90 90: bins 0..3 hold two each; `>` keeps the first three, bin 3 (pairs 6, 7) is cleared -> 6
      hist_tenth_10    ten at rot 0, one at 150: second = 1 against 0.1f * 10 = 1.0: not below, kept -> 11
      hist_tenth_11    eleven at rot 0, one at 150: 1 < 1.1, bin 5 (pair 11) is cleared -> 11
      hist_half        rot 15 twice (15 * (1.0f / 30) = 0.5 exactly in float: round() gives bin 1), rot 30 twice as 10 - 340 = -330 + 360
                       (bin 1), three each at 150, 180, 210 (bins 5, 6, 7): bin 1 holds four and stays with bins 5 and 6; bin 7 (pairs
                       10, 11, 12) is cleared -> 10.  Rounded half to even the two at 15 fall into bin 0 and bins 5, 6, 7 would stay."""
    z = lambda r: (float(r), 0.0)
    return [_pairs([z(0), z(0), z(30), z(30), z(60), z(60), z(90), z(90)], kfkf, "bow_hist_ties", dict(bins_tied_12=1, bins_tied_34=1, cleared_by_histogram=2)),
            _pairs([z(0)] * 10 + [z(150)], kfkf, "bow_hist_tenth_10", dict(second_at_tenth=1)),
            _pairs([z(0)] * 11 + [z(150)], kfkf, "bow_hist_tenth_11", dict(second_below_tenth=1, cleared_by_histogram=1)),
            _pairs([z(15)] * 2 + [(10.0, 340.0)] * 2 + [z(150)] * 3 + [z(180)] * 3 + [z(210)] * 3, kfkf, "bow_hist_half",
                   dict(bin_half=2, rot_negative=2, cleared_by_histogram=3))]


def bow_cases():
    out = []
    for kfkf in (False, True):
        out += bow_size_cases(kfkf)
        out += [bow_taken(kfkf), bow_valid(kfkf), bow_thresholds(kfkf), bow_ratio(kfkf, "075"), bow_ratio(kfkf, "08"), bow_nodes(kfkf)]
        out += bow_hist_cases(kfkf)
    return out


def bow_batches():
    """SearchByBoW(KeyFrame, KeyFrame) of one keyframe against 1, 2 and 5 candidates.  Side 1 is bow_valid's; the candidates:
      V   bow_valid's side 2 with its valid2 -> -1 0 3 5         E   no feature at all -> all -1
      N   V with every node + 1000: no common node -> all -1     A   V with valid2 all ones: node 2 -> 5 at index 2 (5 < 12), node 3 ->
                                                                     best 10, second 12 fails -> -1 0 2 -1
    batch_1 = [V], batch_2 = [E, V], batch_5 = [V, E, N, A, V]."""
    base = bow_valid(True)["args"]

    def cand(kind):
        a = dict(base)
        if kind == "E":
            a.update(desc2=np.zeros((0, 32), np.uint8), node2=np.zeros(0, np.int32), angle2=np.zeros(0, F), valid2=np.zeros(0, np.uint8))
        elif kind == "N":
            a.update(node2=(base["node2"] + 1000).astype(np.int32))
        elif kind == "A":
            a.update(valid2=np.ones_like(base["valid2"]))
        return dict(name="cand_" + kind, kind="bow", forces={}, args=a)
    return [dict(name="bow_batch_%d" % len(ks), kind="bow_batch", forces={}, subs=[cand(k) for k in ks]) for ks in ("V", "EV", "VENAV")]


# ------------------------------------------------------------------------------------------------------------ SearchForTriangulation
SF2 = np.array([1.0, 1.25], F)                             # 100 * scale = 100 and 125
SIGMA_EDGE = np.nextafter(F(1 / 3.84), F(1))               # 0.2604167: 3.84 * it exceeds 1 in double and rounds to 1.0f in float
SIG2 = np.array([1.0, SIGMA_EDGE], F)
ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F)     # a = 0, b = 1, c = -y1: num = y2 - y1, den = 1, dsqr = (y2 - y1)^2


def tri_case(name, groups, F12=ROWS, epipole=(-1000.0, -1000.0), check_ori=False, forces=None):
    """groups: [(node, queries, candidates)], a query = dict(desc, has_mp, x, y, angle), a candidate = the same plus oct."""
    s1, s2 = [], []
    for node, qs, cs in groups:
        s1 += [dict(q, node=node) for q in qs]
        s2 += [dict(c, node=node) for c in cs]
    col = lambda s, k, t: np.array([x[k] for x in s], t)
    a = dict(desc1=np.stack([x["desc"] for x in s1]), node1=col(s1, "node", np.int32), has_mp1=col(s1, "has_mp", np.uint8), x1=col(s1, "x", F),
             y1=col(s1, "y", F), angle1=col(s1, "angle", F), desc2=np.stack([x["desc"] for x in s2]), node2=col(s2, "node", np.int32),
             has_mp2=col(s2, "has_mp", np.uint8), x2=col(s2, "x", F), y2=col(s2, "y", F), angle2=col(s2, "angle", F), octave2=col(s2, "oct", np.int32),
             F12=np.asarray(F12, F), ex=F(epipole[0]), ey=F(epipole[1]), scale_factors2=SF2, level_sigma2_2=SIG2, check_ori=check_ori)
    return dict(name=name, kind="tri", forces=dict(forces or {}), args=a)


def _tq(y=100.0, has_mp=0, angle=0.0, x=200.0):
    return dict(desc=ZERO, has_mp=has_mp, x=x, y=y, angle=angle)


def _tc(d, x=150.0, y=100.0, octave=0, has_mp=0, angle=0.0):
    return dict(desc=near(d), has_mp=has_mp, x=x, y=y, oct=octave, angle=angle)


def tri_size_cases():
    """One query (y = 100) against node ranges of 1, 64, 65 and 129, fillers at 100 (> TH_LOW), every special candidate at 20 on the row
    y = 100 (dsqr = 0) far from the epipole: of equal distances the LAST one that passes both gates stays.
      size_1     the lone candidate -> 0                     size_64    positions 0 and 63 -> 63
      size_65    positions 0 and 64 (the same lane, one stride apart) -> 64
      size_129   positions 5, 70 and 128, and position 127 at 20 but two rows off (dsqr = 4 > 3.84: refused) -> 128"""
    def g(size, special):
        return [(2, [_tq()], [special.get(p, _tc(100)) for p in range(size)])]
    at = lambda *ps: {p: _tc(20) for p in ps}
    s129 = at(5, 70, 128); s129[127] = _tc(20, y=102.0)
    return [tri_case("tri_size_1", g(1, at(0)), forces=dict(max_group2=1)),
            tri_case("tri_size_64", g(64, at(0, 63)), forces=dict(equal_replaces=1)),
            tri_case("tri_size_65", g(65, at(0, 64)), forces=dict(equal_replaces_same_lane=1, equal_replaces_across_stride=1)),
            tri_case("tri_size_129", g(129, s129), forces=dict(equal_replaces=2, equal_replaces_across_stride=2, epipolar_rejected=1, max_group2=129))]


def tri_tie_gates():
    """Epipole (400, 300).  Three nodes, two candidates at distance 20 each; side 2 = [a1 b1 | a2 b2 | a3 b3].
    Node 1 (query y = 100): both on the row, far from the epipole: the later one, b1 -> 1.
    Node 2 (query y = 300): a2 at (150, 300) passes; b2 at (395, 300) is 5 px from the epipole (25 < 100): dropped -> a2 = 2.
    Node 3 (query y = 100): a3 passes; b3 at y = 102 has dsqr = 4 > 3.84 -> a3 = 4."""
    gs = [(1, [_tq()], [_tc(20), _tc(20)]), (2, [_tq(y=300.0)], [_tc(20, y=300.0), _tc(20, x=395.0, y=300.0)]),
          (3, [_tq()], [_tc(20), _tc(20, y=102.0)])]
    return tri_case("tri_tie_gates", gs, epipole=(400.0, 300.0), forces=dict(equal_replaces=1, epipole_rejected=1, epipolar_rejected=1))


def tri_thresholds():
    """A lone candidate at 50 (not above TH_LOW, not above bestDist = TH_LOW: taken -> 0) and one at 51 (-> -1)."""
    return tri_case("tri_thresholds", [(1, [_tq()], [_tc(50)]), (2, [_tq()], [_tc(51)])], forces=dict(dist_eq_th=1, dist_eq_th_plus_1=1))


def tri_epipole():
    """Epipole (400, 0.002f), level 0 (100 * scale = 100), queries at y = 0 (every candidate within 0.002 of its row: dsqr <= 4e-6).
    Node 1: (390, 0.002f): dx = 10, dy = 0: exactly 100, not below -> 0.    Node 2: (390, 0): 100 + 4e-6 rounds to the float above 100 -> 1.
    Node 3: (391, 0): 81 < 100: dropped -> -1."""
    e = float(F(0.002))
    gs = [(1, [_tq(y=0.0)], [_tc(20, x=390.0, y=e)]), (2, [_tq(y=0.0)], [_tc(20, x=390.0, y=0.0)]), (3, [_tq(y=0.0)], [_tc(20, x=391.0, y=0.0)])]
    return tri_case("tri_epipole", gs, epipole=(400.0, e), forces=dict(epipole_at_limit=1, epipole_just_above=1, epipole_rejected=1))


def tri_epipole_level1():
    """Epipole (400, 300), level 1 (100 * 1.25 = 125), queries at y = 295.  (390, 295): 100 + 25 = 125, not below -> 0.  (391, 295): 81 + 25 <
    125: dropped -> -1."""
    gs = [(1, [_tq(y=295.0)], [_tc(20, x=390.0, y=295.0, octave=1)]), (2, [_tq(y=295.0)], [_tc(20, x=391.0, y=295.0, octave=1)])]
    return tri_case("tri_epipole_level1", gs, epipole=(400.0, 300.0), forces=dict(epipole_at_limit=1, epipole_rejected=1))


def tri_den_zero():
    """F12 with nothing but F12[2][2] = 1: a = b = 0, den = 0: CheckDistEpipolarLine returns false -> -1."""
    f = np.zeros((3, 3), F); f[2, 2] = 1
    return tri_case("tri_den_zero", [(1, [_tq()], [_tc(20)])], F12=f, forces=dict(den_zero=1))


def tri_epipolar_sides():
    """Node 1: one row off at level 0 (sigma2 = 1): dsqr = 1 < 3.84 -> 0.   Node 2: two rows off: 4 > 3.84 -> -1.
    Node 3: one row off at level 1, sigma2 = 0.2604167f: 3.84 * sigma2 = 1.0000001 in double, so dsqr = 1 is below it -> 2 (the float product
    3.84f * sigma2 rounds to 1.0f, which 1 is not below)."""
    gs = [(1, [_tq()], [_tc(20, y=101.0)]), (2, [_tq()], [_tc(20, y=102.0)]), (3, [_tq()], [_tc(20, y=101.0, octave=1)])]
    return tri_case("tri_epipolar_sides", gs, forces=dict(epipolar_rejected=1))


def tri_has_mp():
    """Node 1: the query holds a map point: skipped -> -1.  Node 2: the candidate at 10 holds one, the one at 30 does not -> index 2.
    Node 3: two queries, one candidate: vbMatched2 is never set, both take it -> 3, 3."""
    gs = [(1, [_tq(has_mp=1)], [_tc(10)]), (2, [_tq()], [_tc(10, has_mp=1), _tc(30)]), (3, [_tq(), _tq()], [_tc(20)])]
    return tri_case("tri_has_mp", gs, forces=dict(skipped_has_mp1=1, skipped_has_mp2=1))


def tri_hist(check_ori):
    """bow_hist_ties' rotations on lone pairs: with the orientation check pairs 6 and 7 (bin 3) are cleared -> 6, without it all 8 stay."""
    gs = [(i, [_tq(angle=float(r))], [_tc(20)]) for i, r in enumerate((0, 0, 30, 30, 60, 60, 90, 90))]
    return tri_case("tri_hist_%s" % ("on" if check_ori else "off"), gs, check_ori=check_ori,
                    forces=dict(bins_tied_12=1, cleared_by_histogram=2) if check_ori else {})


def tri_cases():
    return tri_size_cases() + [tri_tie_gates(), tri_thresholds(), tri_epipole(), tri_epipole_level1(), tri_den_zero(), tri_epipolar_sides(),
                               tri_has_mp(), tri_hist(True), tri_hist(False)]


# ------------------------------------------------------------------------------------------------------------ all of them
def descent_cases():
    out = [descent(o) for o in ORDERS] + [descent("depth_first", L=4), descent("interleaved", L=4), descent_extremes()]
    out += [descent("depth_first", levelsups=[0, 1], n=n) for n in (1, 255, 256, 257, 4096, 4097)]    # 4096 / 4097: the directory on the device / host
    return out


def small_cases():
    """Everything but the grid vocabulary's cases (whose answers are closed forms)."""
    return (descent_cases() + [bowvec_weights(), bowvec_many_hits(), bowvec_all_stopped(), scores()] + distinctive_calls() + directory_cases() +
            bow_cases() + bow_batches() + tri_cases())


def all_cases():
    return small_cases() + grid_cases()


def run_ref(case, *, wrong=(), trace=None):
    """The definition's answer for a case."""
    k, a = case["kind"], case.get("args")
    kw = dict(wrong=wrong, trace=trace)
    if k == "descent":
        voc = R.Vocabulary(a["k"], a["L"], a["parent"], a["desc"], a["weight"], wrong=wrong)
        out = []
        for lu in a["levelsups"]:                                    # Frame::ComputeBoW: the transform, the FeatureVector nodes, their directory
            wid, w, nid = voc.transform_features(a["feats"], lu, **kw)
            fv = R.bow_vector(wid, w, nid, **kw)[2]
            out.append([wid, w, nid, fv] + list(R.feature_vector(fv)))
        return out
    if k == "grid":
        v = a["voc"]
        voc = R.Vocabulary(v["k"], v["L"], v["parent"], v["desc"], v["weight"], wrong=wrong)
        wid, w, nid = voc.transform_features(a["feats"], a["levelsup"], **kw)
        _, _, fv = R.bow_vector(wid, w, nid, **kw)
        return [wid, w, fv] + list(R.feature_vector(fv))
    if k == "bowvec":
        return [R.bow_vector(a["word_id"], a["weight"], a["node_id"], wt, sc, **kw) for wt, sc in COMBOS]
    if k == "score":
        return [R.score_l1(x, y) for x, y in a["pairs"]]
    if k == "distinctive":
        return [R.distinctive(g, **kw) for g in a["groups"]]
    if k == "directory":
        return [R.feature_vector(p) for p in a["patterns"].values()]
    if k == "bow":
        return R.search_by_bow(a["desc1"], a["node1"], a["valid1"], a["angle1"], a["desc2"], a["node2"], a["angle2"], a["valid2"], a["nnratio"],
                               a["check_ori"], a["kfkf"], **kw)
    if k == "bow_batch":
        return [run_ref(s, **kw) for s in case["subs"]]
    assert k == "tri"
    return R.search_for_triangulation(a["desc1"], a["node1"], a["has_mp1"], a["x1"], a["y1"], a["angle1"], a["desc2"], a["node2"], a["has_mp2"],
                                      a["x2"], a["y2"], a["angle2"], a["octave2"], a["F12"], a["ex"], a["ey"], a["scale_factors2"], a["level_sigma2_2"],
                                      a["check_ori"], **kw)
