"""The matrix-core Hamming matcher -- FP4 operands through the block-scaled matrix instruction -- against the CPU oracle, bit for
bit, and a known-answer test of the FP4 tile itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(d):
    return np.unpackbits(np.ascontiguousarray(d, np.uint8), axis=-1, bitorder="little").astype(np.int64)


def _tile(ctx, a, b, c):
    from motioncheck_ccm_slam_amd import _lib
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8); c = np.ascontiguousarray(c, np.float32)
    assert a.shape == (32, 32) and b.shape == (32, 32) and c.shape == (32,)
    out = np.full((32, 32), np.nan, np.float32)
    ctx.check(_lib.load().ccm_debug_fp4_tile(ctx.handle, _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(out)))
    return out


def _expect(a, b, c):
    """row_c[i] - 4096 * <a_i, b_j> in integers (numpy), as float32: every value is an integer below 2^24, so float32 holds it."""
    want = c.astype(np.int64)[:, None] - 4096 * (_bits(a) @ _bits(b).T)
    assert (np.abs(want) < 1 << 24).all()
    return want.astype(np.float32)


def _single(bit):
    d = np.zeros(32, np.uint8)
    d[bit >> 3] = 1 << (bit & 7)
    return d


def test_fp4_tile_known_answers(ctx):
    """Hand-built 32 x 32 operands: the e2m1 encodings (+1.0 trains, -1.0 queries), the E8M0 scales (a single common bit is exactly
    -4096), the k assignment of A and B (every one of the 256 bit positions meets itself and nothing else), the C operand, and
    the exactness bound (the largest and smallest keys the matcher can produce)."""
    zeros = np.zeros(32, np.float32)
    # one common bit: -4096 on the diagonal and nowhere else, for every bit position
    for k in range(8):
        a = np.stack([_single(32 * k + i) for i in range(32)])
        out = _tile(ctx, a, a, zeros)
        assert (out == -4096.0 * np.eye(32, dtype=np.float32)).all(), k
        b = np.stack([_single((32 * k + 37 * j + 5) % 256) for j in range(32)])          # other positions: only true coincidences count
        assert (_tile(ctx, a, b, zeros) == _expect(a, b, zeros)).all(), k
    # all-zero and all-one rows on either side: dot products 0 and 256
    a = np.zeros((32, 32), np.uint8); b = np.zeros((32, 32), np.uint8)
    a[1::2] = 255; b[::3] = 255; a[5, :16] = 0; b[6, 16:] = 0
    c = np.arange(32, dtype=np.float32) * 3 + 7
    out = _tile(ctx, a, b, c)
    assert (out == _expect(a, b, c)).all()
    assert out[1, 0] == c[1] - 4096 * 256 and out[0, 0] == c[0] and out[1, 1] == c[1]
    # the matcher's row words: (popc + 4352) << 11 | index with the largest index field, random and extreme rows
    rng = np.random.default_rng(11)
    for trial in range(4):
        a = rng.integers(0, 256, (32, 32), dtype=np.uint8); b = rng.integers(0, 256, (32, 32), dtype=np.uint8)
        a[0] = 255; b[0] = 255; a[1] = 0; b[1] = 0; b[2] = a[3]; b[4] = ~a[4]
        idx = 2047 - np.arange(32) * trial
        c = (((_bits(a).sum(1) + 4352) << 11) | idx).astype(np.float32)
        assert c.max() < 1 << 24
        out = _tile(ctx, a, b, c)
        assert (out == _expect(a, b, c)).all(), trial
        assert out[0, 1] == float(((256 + 4352) << 11) | 2047)                          # the largest key: all-one train, no common bit
        assert out[0, 0] == float(((4352 - 256) << 11) | 2047)                          # the smallest distance field


def _check(m, oracle, q, t, nq_n=None, nt_n=None):
    bi, bd, sd = m.BruteForce(q, t, nq_n, nt_n)
    q3 = q if q.ndim == 3 else q[None]; t3 = t if t.ndim == 3 else t[None]
    for p in range(len(q3)):
        nqp = q3.shape[1] if nq_n is None else int(nq_n[p]); ntp = t3.shape[1] if nt_n is None else int(nt_n[p])
        if nqp:
            rbi, rbd, rsd = oracle.hamming_match(q3[p, :nqp], t3[p, :ntp])
            assert (bi[p, :nqp] == rbi).all(), ("best index", p, nqp, ntp)
            assert (bd[p, :nqp] == rbd).all(), ("best distance", p, nqp, ntp)
            assert (sd[p, :nqp] == rsd).all(), ("second distance", p, nqp, ntp)
        assert (bi[p, nqp:] == -1).all() and (bd[p, nqp:] == 256).all() and (sd[p, nqp:] == 256).all(), ("rows past the live count", p)
    return bi, bd, sd


def run_cases(ctx, oracle):
    """Best index, best distance and second distance EXACTLY as the oracle's hamming_match."""
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    m = ORBmatcher(ctx=ctx)
    rng = np.random.default_rng(2024)
    rand = lambda *shape: rng.integers(0, 256, shape + (32,), dtype=np.uint8)

    # all-zero and all-one descriptors on either side: dot products 0 and 256, popcounts 0 and 256
    for nq, nt in ((4, 4), (70, 45)):
        for qv in (0, 255):
            for tv in (0, 255):
                bi, bd, sd = _check(m, oracle, np.full((nq, 32), qv, np.uint8), np.full((nt, 32), tv, np.uint8))
                assert (bd == (0 if qv == tv else 256)).all() and (bi == (0 if qv == tv else -1)).all()
    q = rand(50); t = rand(90)
    q[3] = 0; q[4] = 255; t[10] = 0; t[11] = 255; t[50] = 0; t[51] = 255
    _check(m, oracle, q, t)

    # identical rows repeated: the lowest index wins, second == best
    t = rand(300)
    for k in (33, 64, 200, 250, 299):
        t[k] = t[17]
    t[40:72] = t[5]                                                     # a whole tile of copies, over a tile border
    q = t[[17, 5, 250, 41, 0]].copy()
    q[4, 0] ^= 1
    bi, bd, sd = _check(m, oracle, q, t)
    assert bi[0, 0] == 17 and bd[0, 0] == 0 and sd[0, 0] == 0 and bi[0, 1] == 5 and bi[0, 2] == 17 and bi[0, 3] == 5
    _check(m, oracle, np.repeat(rand(1), 77, 0), np.repeat(rand(1), 131, 0))      # every distance equal: index 0 everywhere

    # train counts around the 32-row tile and at the limits of the matrix-core kernel; query counts off the 32 / 256 grid
    for nt in (1, 31, 32, 33, 1000, 2047, 2048):
        for nq in (1, 37, 300):
            t = rand(nt); q = rand(nq)
            q[0] = t[nt - 1]                                            # the last train row is seen
            if nq > 1:
                q[nq // 2] = t[nt // 2]; q[nq // 2, 31] ^= 0x81         # planted near-duplicate (2 bits)
            bi, bd, sd = _check(m, oracle, q, t)
            assert bd[0, 0] == 0
    _check(m, oracle, rand(1001), rand(999))

    # live counts 0 and below the padded size, several pairs with differing counts
    q = rand(7, 530); t = rand(7, 1200)
    nq_n = np.array([530, 257, 1, 0, 31, 300, 529]); nt_n = np.array([1200, 33, 1, 77, 0, 1199, 32])
    t[0, 1100] = q[0, 500]; t[5, 64] = q[5, 299]; t[5, 1198] = q[5, 299]
    bi, bd, sd = _check(m, oracle, q, t, nq_n, nt_n)
    assert bi[0, 500] == 1100 and bi[5, 299] == 64 and sd[5, 299] == 0 and (bi[4] == -1).all() and (sd[2, :1] == 256).all()
    _check(m, oracle, rand(2, 40), rand(2, 100), None, np.array([0, 100]))
    _check(m, oracle, rand(2, 40), rand(2, 100), np.array([40, 0]), None)
    bi, bd, sd = m.BruteForce(rand(10), rand(10)[:0])                   # no train rows at all
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()

    # random descriptors with planted near-duplicates: k flipped bits, twice for a close second
    q = rand(3, 900); t = rand(3, 1000)
    for p in range(3):
        slot = iter(rng.permutation(1000))                              # (no planted row lands on another)
        for i in range(0, 900, 3):
            d = q[p, i].copy()
            for bit in rng.choice(256, int(rng.integers(0, 30)), replace=False):
                d[bit >> 3] ^= 1 << (bit & 7)
            t[p, next(slot)] = d
            if i % 2 == 0:
                d2 = d.copy(); d2[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
                t[p, next(slot)] = d2
    bi, bd, sd = _check(m, oracle, q, t)
    assert (bd[:, ::3] < 40).mean() > 0.9


def test_matrix_core_matcher_matches_oracle_exactly(ctx, oracle):
    run_cases(ctx, oracle)
