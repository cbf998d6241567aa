// init_math_check.cpp -- csrc/init_math.h on the host: what k_init_hypotheses computes per hypothesis, lane by lane in a loop (the
// two halves of each Jacobi rotation for all 9 owners in turn, the score as 64 per-lane sums and the kernel's xor tree).
// stdin:  int32 n, iters; float T1[4], T2[4], inv_sigma2; float m[n][4]; int32 sets[iters][8]
// stdout: float H21[iters][9], H12[iters][9], F21[iters][9], score_h[iters], score_f[iters]; uint8 in_h[iters][n], in_f[iters][n];
//         int32 rotations[iters][2]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/init_types.h"
#include "../../motioncheck_ccm_slam_amd/csrc/init_math.h"

template <class T> static bool rd(T* p, size_t n) { return fread(p, sizeof(T), n, stdin) == n; }
template <class T> static void wr(const T* p, size_t n) { fwrite(p, sizeof(T), n, stdout); }

int main()
{
    int32_t n, iters; float T1[4], T2[4], inv_sigma2;
    if (!rd(&n, 1) || !rd(&iters, 1) || !rd(T1, 4) || !rd(T2, 4) || !rd(&inv_sigma2, 1) || n < 8 || iters < 1) return 2;
    std::vector<float> m(4 * (size_t)n); std::vector<int32_t> sets(8 * (size_t)iters);
    if (!rd(m.data(), m.size()) || !rd(sets.data(), sets.size())) return 2;
    std::vector<float> H21(9 * (size_t)iters), H12(H21.size()), F21(H21.size()), sh(iters), sf(iters);
    std::vector<uint8_t> in_h((size_t)iters * n), in_f(in_h.size());
    std::vector<int32_t> rotations(2 * (size_t)iters);
    for (int it = 0; it < iters; it++)
        for (int isF = 0; isF < 2; isF++) {
            float A[16][9]; double M[81], V[81];
            for (int c = 0; c < 16; c++) {
                const float* mm = m.data() + 4 * (size_t)sets[8 * it + (isF ? (c & 7) : (c >> 1))];
                const float u1 = (mm[0] - T1[2]) * T1[0], v1 = (mm[1] - T1[3]) * T1[1], u2 = (mm[2] - T2[2]) * T2[0], v2 = (mm[3] - T2[3]) * T2[1];
                if (isF) { ini_row_f(u1, v1, u2, v2, A[c]); if (c >= 8) for (int k = 0; k < 9; k++) A[c][k] = 0; }
                else ini_row_h(c, u1, v1, u2, v2, A[c]);
            }
            for (int c = 0; c < 9; c++)
                for (int j = 0; j < 9; j++) {
                    double acc = 0;
                    for (int r = 0; r < 16; r++) acc += (double)A[r][c] * (double)A[r][j];
                    M[9 * c + j] = acc; V[9 * c + j] = c == j;
                }
            int rot = 0;
            for (int sweep = 0; sweep < INI_SWEEPS; sweep++)
                for (int p = 0; p < 8; p++)
                    for (int q = p + 1; q < 9; q++) {
                        const double app = M[9 * p + p], aqq = M[9 * q + q], apq = M[9 * p + q];
                        if (ini_negligible(app, aqq, apq)) continue;
                        rot++;
                        double cs, sn;
                        ini_rotation(app, aqq, apq, &cs, &sn);
                        for (int k = 0; k < 9; k++) ini_jacobi9_row(M, V, k, p, q, cs, sn);
                        for (int k = 0; k < 9; k++) ini_jacobi9_col(M, k, p, q, cs, sn);
                    }
            rotations[2 * it + isF] = rot;
            const int jmin = ini_jacobi9_smallest(M);
            double x[9];
            for (int k = 0; k < 9; k++) x[k] = V[9 * k + jmin];
            float A0[9], A1[9];
            if (isF) ini_finish_f(x, T1, T2, A0); else ini_finish_h(x, T1, T2, A0, A1);
            memcpy((isF ? F21 : H21).data() + 9 * (size_t)it, A0, 36);
            if (!isF) memcpy(H12.data() + 9 * (size_t)it, A1, 36);
            float part[64] = { 0 };
            for (int i = 0; i < n; i++) {
                const float* mm = m.data() + 4 * (size_t)i; bool in; float s1, s2;
                if (isF) ini_check_f(A0, mm[0], mm[1], mm[2], mm[3], inv_sigma2, &in, &s1, &s2);
                else ini_check_h(A0, A1, mm[0], mm[1], mm[2], mm[3], inv_sigma2, &in, &s1, &s2);
                part[i & 63] += s1; part[i & 63] += s2;
                (isF ? in_f : in_h)[(size_t)it * n + i] = in;
            }
            for (int o = 32; o >= 1; o >>= 1) {
                float t[64];
                for (int l = 0; l < 64; l++) t[l] = part[l] + part[l ^ o];
                memcpy(part, t, sizeof t);
            }
            (isF ? sf : sh)[it] = part[0];
        }
    wr(H21.data(), H21.size()); wr(H12.data(), H12.size()); wr(F21.data(), F21.size()); wr(sh.data(), sh.size()); wr(sf.data(), sf.size());
    wr(in_h.data(), in_h.size()); wr(in_f.data(), in_f.size()); wr(rotations.data(), rotations.size());
    return 0;
}
