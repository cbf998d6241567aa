// match_bf_host.cpp -- C ABI of the brute-force Hamming search (include/ccm_hot.h) and the matcher's scalar helpers.
#include "match_internal.h"
#include <algorithm>

void match_state_free(MatchState* s) { delete s; }

extern "C" {

// ORBmatcher::DescriptorDistance, ORBmatcher.cpp:1653-1669
int ccm_descriptor_distance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

// ORBmatcher.cpp:247-249 (Frame overload) / :641-643 (KF-KF overload)
int ccm_ratio_test(int best_dist, int second_dist, float nnratio, int th, int strict)
{
    const bool pass = strict ? (best_dist < th) : (best_dist <= th);
    return pass && (static_cast<float>(best_dist) < nnratio * static_cast<float>(second_dist)) ? 1 : 0;
}

int ccm_hamming_match_dev(ccm_ctx* c, const uint8_t* q_dev, int nq, size_t q_pair_stride, const uint8_t* t_dev, int nt,
                          size_t t_pair_stride, int n_pairs, const int32_t* nq_n_dev, const int32_t* nt_n_dev,
                          int32_t* best_idx_dev, int32_t* best_dist_dev, int32_t* second_dist_dev)
{
    RoctxRange roctx_("ccm_hamming_match_dev");
    return ccm_guard(c, "ccm_hamming_match_dev", [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (n_pairs == 0 || nq == 0) return CCM_OK;
        if (n_pairs < 0 || nq < 0 || nt < 0 || nt > 65535 || !q_dev || (!t_dev && nt > 0) || !best_idx_dev || !best_dist_dev || !second_dist_dev)
            return ccm_fail(c, CCM_E_ARG, "bad matcher arguments (nt must be <= 65535)");
        if (((uintptr_t)q_dev | (uintptr_t)t_dev) & 15) return ccm_fail(c, CCM_E_ARG, "descriptor arrays must be 16-byte aligned");
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        // Few pairs cannot fill 256 CUs with one workgroup each: split the train rows of a pair over several
        // workgroups (exact merge afterwards) until there are about four workgroups per CU.
        // (Only the vector-ALU kernel splits: the matrix-core kernel, which takes every nt <= 2048, ignores n_split.)
        int n_split = 1;
        while (n_split < 8 && (long long)n_pairs * n_split < 1024 && nt / (n_split * 2) >= 128) n_split *= 2;
        if (n_split > 1) {
            CCM_RESERVE(c, M.part_best, (size_t)n_pairs * n_split * nq * 4);
            CCM_RESERVE(c, M.part_second, (size_t)n_pairs * n_split * nq * 4);
        }
        ProfScope ps(c, CCM_PROF_HAMMING_BF);
        match_launch_bf(c->stream, q_dev, (long long)q_pair_stride * 32, t_dev, (long long)t_pair_stride * 32, nq, nt, n_pairs,
                        nq_n_dev, nt_n_dev, n_split, M.part_best.as<unsigned>(), M.part_second.as<int>(),
                        best_idx_dev, best_dist_dev, second_dist_dev);
        CCM_HIP(c, hipGetLastError());
        return CCM_OK;
    });
}

int ccm_hamming_match(ccm_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, int n_pairs, const int32_t* nq_n,
                      const int32_t* nt_n, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist)
{
    RoctxRange roctx_("ccm_hamming_match");
    return ccm_guard(c, "ccm_hamming_match", [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (n_pairs == 0 || nq == 0) return CCM_OK;
        if (n_pairs < 0 || nq < 0 || nt < 0 || !q || (!t && nt > 0) || !best_idx || !best_dist || !second_dist)
            return ccm_fail(c, CCM_E_ARG, "bad matcher arguments");
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        const size_t qb = (size_t)n_pairs * nq * 32, tb = (size_t)n_pairs * nt * 32, ob = (size_t)n_pairs * nq * 4;
        CCM_RESERVE(c, M.q, qb); CCM_RESERVE(c, M.t, std::max<size_t>(tb, 32));
        CCM_RESERVE(c, M.bi, ob); CCM_RESERVE(c, M.bd, ob); CCM_RESERVE(c, M.sd, ob);
        CCM_RESERVE(c, M.nqn, (size_t)n_pairs * 4); CCM_RESERVE(c, M.ntn, (size_t)n_pairs * 4);
        CCM_HIP(c, hipMemcpyAsync(M.q.p, q, qb, hipMemcpyHostToDevice, c->stream));
        if (tb) CCM_HIP(c, hipMemcpyAsync(M.t.p, t, tb, hipMemcpyHostToDevice, c->stream));
        if (nq_n) CCM_HIP(c, hipMemcpyAsync(M.nqn.p, nq_n, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        if (nt_n) CCM_HIP(c, hipMemcpyAsync(M.ntn.p, nt_n, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        int rc = ccm_hamming_match_dev(c, M.q.as<uint8_t>(), nq, nq, M.t.as<uint8_t>(), nt, nt, n_pairs,
                                       nq_n ? M.nqn.as<int32_t>() : nullptr, nt_n ? M.ntn.as<int32_t>() : nullptr,
                                       M.bi.as<int32_t>(), M.bd.as<int32_t>(), M.sd.as<int32_t>());
        if (rc) return rc;
        CCM_HIP(c, hipMemcpyAsync(best_idx, M.bi.p, ob, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipMemcpyAsync(best_dist, M.bd.p, ob, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipMemcpyAsync(second_dist, M.sd.p, ob, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        return CCM_OK;
    });
}

int ccm_debug_fp4_tile(ccm_ctx* c, const uint8_t* a, const uint8_t* b, const float* row_c, float* out)
{
    return ccm_guard(c, "ccm_debug_fp4_tile", [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (!a || !b || !row_c || !out) return ccm_fail(c, CCM_E_ARG, "bad FP4 tile arguments");
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        int rc;
        if ((rc = ccm_upload(c, M.q, a, 1024, c->stream)) || (rc = ccm_upload(c, M.t, b, 1024, c->stream)) || (rc = ccm_upload(c, M.bd, row_c, 128, c->stream))) return rc;
        CCM_RESERVE(c, M.sd, 4096);
        match_launch_fp4_tile(c->stream, M.q.as<unsigned>(), M.t.as<unsigned>(), M.bd.as<float>(), M.sd.as<float>());
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(out, M.sd.p, 4096, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        return CCM_OK;
    });
}
}  // extern "C"
