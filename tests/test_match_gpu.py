"""HIP Hamming matcher vs the CPU oracle through the C ABI (BASELINE config 3) and SearchByBoW.  test_search_by_bow runs on random
descriptor pairs, where Hamming ties and threshold equalities do not occur; the oracle's SearchByBoW is held to tests/bow_ref.py (the
definition restated from the reference's text) on the same inputs by tests/test_bow_cases_cpu.py, and the tie, threshold, ratio and
taken-candidate rules are forced by the hand-built cases of tests/test_bow_cases_gpu.py."""
import os

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import synth
from motioncheck_ccm_slam_amd.matcher import ORBmatcher
import bow_inputs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_pairs_match_oracle_and_fixture(ctx, oracle):
    m = ORBmatcher(0.7, ctx=ctx)
    q, t = synth.descriptor_pairs(0, 8)
    bi, bd, sd = m.BruteForce(q, t)
    for p in range(8):
        rbi, rbd, rsd = oracle.hamming_match(q[p], t[p])
        assert (bi[p] == rbi).all() and (bd[p] == rbd).all() and (sd[p] == rsd).all()
    z = np.load(os.path.join(G, "match_pair0.npz"))
    assert (bi[0] == z["best_idx"]).all() and (bd[0] == z["best_dist"]).all() and (sd[0] == z["second_dist"]).all()
    # ratio test of the callers
    ok = m.RatioTest(bd[0], sd[0])
    assert ok.sum() > 600 and ((bd[0] <= 50) | ~ok).all()


def test_ties_pick_lowest_index(ctx, oracle):
    m = ORBmatcher(ctx=ctx)
    rng = np.random.default_rng(1)
    t = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    t[200] = t[17]; t[250] = t[17]                # duplicates: the first index must win, second == best
    q = t[[17, 5, 250]].copy()
    q[1, 0] ^= 1
    bi, bd, sd = m.BruteForce(q, t)
    rbi, rbd, rsd = oracle.hamming_match(q, t)
    assert (bi[0] == rbi).all() and (bd[0] == rbd).all() and (sd[0] == rsd).all()
    assert bi[0, 0] == 17 and bd[0, 0] == 0 and sd[0, 0] == 0


def test_ragged_empty_and_tiled(ctx, oracle):
    m = ORBmatcher(ctx=ctx)
    rng = np.random.default_rng(2)
    q = rng.integers(0, 256, (3, 1300, 32), dtype=np.uint8)        # > 1024 queries: two query passes
    t = rng.integers(0, 256, (3, 2500, 32), dtype=np.uint8)        # > 1024 train rows: three LDS tiles
    nq_n = np.array([1300, 7, 0]); nt_n = np.array([2500, 1025, 300])
    bi, bd, sd = m.BruteForce(q, t, nq_n, nt_n)
    for p in range(3):
        rbi, rbd, rsd = oracle.hamming_match(q[p, :nq_n[p]], t[p, :nt_n[p]])
        assert (bi[p, :nq_n[p]] == rbi).all() and (bd[p, :nq_n[p]] == rbd).all() and (sd[p, :nq_n[p]] == rsd).all()
        assert (bi[p, nq_n[p]:] == -1).all() and (bd[p, nq_n[p]:] == 256).all()
    bi, bd, sd = m.BruteForce(q[:1, :10], t[:1, :0])               # no train rows at all
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()
    allz = np.zeros((1, 4, 32), np.uint8); allo = np.full((1, 4, 32), 255, np.uint8)
    bi, bd, sd = m.BruteForce(allz, allo)                          # distance 256 is never a match (strict <)
    assert (bi == -1).all() and (bd == 256).all()


def test_ragged_counts_below_2048_trains(ctx, oracle):
    """The matrix-core kernel's range (<= 2048 train rows): partial last tiles, dead query blocks, one train, none."""
    m = ORBmatcher(ctx=ctx)
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (6, 1100, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (6, 1500, 32), dtype=np.uint8)
    t[0, 40] = q[0, 3]; t[0, 900] = q[0, 3]                         # duplicate best: the lower index wins, second = 0
    nq_n = np.array([1100, 257, 1, 0, 700, 64]); nt_n = np.array([1500, 33, 1, 77, 0, 1024])
    bi, bd, sd = m.BruteForce(q, t, nq_n, nt_n)
    for p in range(6):
        rbi, rbd, rsd = oracle.hamming_match(q[p, :nq_n[p]], t[p, :nt_n[p]])
        assert (bi[p, :nq_n[p]] == rbi).all() and (bd[p, :nq_n[p]] == rbd).all() and (sd[p, :nq_n[p]] == rsd).all(), p
        assert (bi[p, nq_n[p]:] == -1).all() and (bd[p, nq_n[p]:] == 256).all() and (sd[p, nq_n[p]:] == 256).all()
    assert bi[0, 3] == 40 and bd[0, 3] == 0 and sd[0, 3] == 0
    assert (sd[2, :1] == 256).all() and (bi[4, :700] == -1).all()


def test_vector_alu_kernel_splits_and_unsplit(ctx, oracle):
    """One train row past the matrix-core limit (2049: the third LDS tile of k_hamming_bf holds one row) at 1024, 512 and 256
    pairs, where the split rule gives 1 (the unsplit write path), 2 and 4 workgroups per pair; ragged counts including empty sides;
    a query duplicated at the last live train row and at an earlier one (other tile, other split): the lower index wins and
    second == best.  Exact against the oracle for every live row, the defaults past the live counts."""
    m = ORBmatcher(ctx=ctx)
    rng = np.random.default_rng(7)
    NP, NQ, NT = 1024, 5, 2049
    q = rng.integers(0, 256, (NP, NQ, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (NP, NT, 32), dtype=np.uint8)
    nt_n = rng.integers(0, NT + 1, NP); nq_n = rng.integers(0, NQ + 1, NP)
    corner = [(a, b) for a in (2049, 2048, 1025, 1, 0) for b in (5, 1, 0)]               # every pairing, inside the 256-pair slice
    nt_n[:len(corner)] = [a for a, b in corner]; nq_n[:len(corner)] = [b for a, b in corner]
    planted = (nt_n >= 2) & (nq_n >= 1)
    early = (nt_n - 1) // 2
    for p in np.flatnonzero(planted):
        t[p, nt_n[p] - 1] = q[p, 0]; t[p, early[p]] = q[p, 0]
    assert planted[0] and early[0] == 1024 and planted[:256].sum() > 100
    want = [oracle.hamming_match(q[p, :nq_n[p]], t[p, :nt_n[p]]) if nq_n[p] else None for p in range(NP)]
    for n_pairs in (1024, 512, 256):
        bi, bd, sd = m.BruteForce(q[:n_pairs], t[:n_pairs], nq_n[:n_pairs], nt_n[:n_pairs])
        for p in range(n_pairs):
            n = nq_n[p]
            if n:
                rbi, rbd, rsd = want[p]
                assert (bi[p, :n] == rbi).all() and (bd[p, :n] == rbd).all() and (sd[p, :n] == rsd).all(), (n_pairs, p, n, nt_n[p])
            assert (bi[p, n:] == -1).all() and (bd[p, n:] == 256).all() and (sd[p, n:] == 256).all(), (n_pairs, p)
        sel = planted[:n_pairs]
        assert (bi[:n_pairs, 0][sel] == early[:n_pairs][sel]).all() and (bd[:n_pairs, 0][sel] == 0).all() and (sd[:n_pairs, 0][sel] == 0).all()


def test_many_pairs_property(ctx, oracle):
    """A 512-pair slice of config 3 through the host-buffer entry point (ORBmatcher.BruteForce): symmetric checks on all,
    oracle on a sample.  The full 10,000 pairs are the next test."""
    m = ORBmatcher(0.7, ctx=ctx)
    q, t = synth.descriptor_pairs(100, 512)
    bi, bd, sd = m.BruteForce(q, t)
    assert ((bi >= 0) & (bi < 1000)).all() and (bd <= sd).all()
    # the reported best distance is the true distance to the reported index
    sel = np.take_along_axis(t, bi[:, :, None].astype(np.int64), axis=1)
    true = np.unpackbits(q ^ sel, axis=2).sum(2)
    assert (true == bd).all()
    for p in (0, 100, 511):
        rbi, rbd, rsd = oracle.hamming_match(q[p], t[p])
        assert (bi[p] == rbi).all() and (sd[p] == rsd).all()


def test_config3_all_10000_pairs(ctx, oracle):
    """BASELINE config 3 at its stated size: 10,000 pairs of 1000 x 1000 descriptors (seeds 0xDE5C0000 + p), generated on the
    device by the torch twin of synth.descriptor_pairs (bit-identical, tests/test_synth_cpu.py), matched in ONE launch of the
    device-resident entry point as bench.py's match_10k leg does.  Size-independent properties on every pair -- index range,
    best <= second, the reported best distance IS the distance to the reported index, no sampled train row is closer, the
    planted inlier is found -- and bit equality with the oracle on 20 pairs spread over the whole range."""
    import ctypes as C
    import torch
    from motioncheck_ccm_slam_amd import _lib
    lib = _lib.load()
    NP = 10000
    qa, tb = synth.descriptor_pairs_torch(0, NP, device="cuda")
    bi = torch.empty((NP, 1000), dtype=torch.int32, device="cuda"); bd = torch.empty_like(bi); sd = torch.empty_like(bi)
    torch.cuda.synchronize()
    ctx.check(lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(qa.data_ptr()), 1000, C.c_size_t(1000), C.c_void_p(tb.data_ptr()), 1000,
                                        C.c_size_t(1000), NP, None, None, C.c_void_p(bi.data_ptr()), C.c_void_p(bd.data_ptr()), C.c_void_p(sd.data_ptr())))
    ctx.sync()
    assert bool(((bi >= 0) & (bi < 1000)).all()) and bool((bd <= sd).all()) and bool((bd >= 0).all()) and bool((sd <= 256).all())
    lut = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int16, device="cuda")
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    n_inlier_hits = 0
    for p0 in range(0, NP, 500):
        q = qa[p0:p0 + 500]; t = tb[p0:p0 + 500]; idx = bi[p0:p0 + 500].long()
        sel = torch.gather(t, 1, idx[:, :, None].expand(-1, -1, 32))
        true = lut[(q ^ sel).long()].sum(-1, dtype=torch.int32)
        assert bool((true == bd[p0:p0 + 500]).all()), p0
        rnd = torch.randint(0, 1000, (500, 1000), device="cuda", generator=g)
        other = torch.gather(t, 1, rnd[:, :, None].expand(-1, -1, 32))
        d_other = lut[(q ^ other).long()].sum(-1, dtype=torch.int32)
        assert bool((d_other >= bd[p0:p0 + 500]).all()), p0                       # nothing sampled beats the reported best
        assert bool(((d_other >= sd[p0:p0 + 500]) | (rnd == idx)).all()), p0      # and nothing but the best beats the second
        n_inlier_hits += int((bd[p0:p0 + 500] < 40).sum())
    assert n_inlier_hits > 0.6 * NP * 1000                                        # 70 % of the rows carry a planted match at ~15 bits
    for p in list(range(0, NP, 625)) + [1, 4999, 5000, 9999]:
        rbi, rbd, rsd = oracle.hamming_match(qa[p].cpu().numpy(), tb[p].cpu().numpy())
        assert (bi[p].cpu().numpy() == rbi).all() and (bd[p].cpu().numpy() == rbd).all() and (sd[p].cpu().numpy() == rsd).all(), p


@pytest.mark.parametrize("kfkf", [False, True])
def test_search_by_bow(ctx, oracle, kfkf):
    i = bow_inputs.search_by_bow(oracle, kfkf)
    d1, d2, node1, node2, v1, v2, ang1, ang2 = (i[k] for k in ("d1", "d2", "node1", "node2", "v1", "v2", "ang1", "ang2"))
    n1, n2 = len(d1), len(d2)
    for ratio, ori in ((0.7, True), (0.75, True), (0.9, False)):
        m = ORBmatcher(ratio, ori, ctx=ctx)
        n, mt = m.SearchByBoW(d1, node1, v1, ang1, d2, node2, ang2, valid2=v2)
        rn, rm = oracle.match_bow(ratio, int(ori), 50, int(kfkf), d1, node1, v1, ang1, d2, node2, v2, ang2)
        assert n == rn and (mt == rm).all()
        assert n > 100
    # one node holding everything == brute force with greedy exclusion
    m = ORBmatcher(0.7, True, ctx=ctx)
    z1 = np.zeros(n1, int); z2 = np.zeros(n2, int)
    n, mt = m.SearchByBoW(d1, z1, v1, ang1, d2, z2, ang2, valid2=v2)
    rn, rm = oracle.match_bow(0.7, 1, 50, int(kfkf), d1, z1, v1, ang1, d2, z2, v2, ang2)
    assert n == rn and (mt == rm).all()
    # empty sides
    n, mt = m.SearchByBoW(d1[:0], z1[:0], v1[:0], ang1[:0], d2, z2, ang2, valid2=v2)
    assert n == 0 and len(mt) == 0
