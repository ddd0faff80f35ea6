// softdtw.hip -- batched soft-DTW (Cuturi & Blondel 2017) over cosine cells and its gradient (abnq_softdtw_forward,
// abnq_softdtw_backward).  include/abnet3_hip_next.h states the definition, tests/sdtw_np.py restates it, DESIGN.md
// section 3.4i has the phases, the workspace and the measurements.
//
// A workgroup of four waves per problem (a grid-stride loop over the problems), three phases a call:
//   forward   1. a wave per row: the norm in float64; 1 / max(|x|, 1e-6) and |x| go to the workspace.
//             2. all four waves: c[i][j] = <x_i, y_j> / (max(|x_i|, 1e-6) max(|y_j|, 1e-6)), 2 x 2 tiles a thread
//                (dtw_wave.h's tiling), the dot product a float64 fma chain in k order over the raw float32 rows, the cell
//                rounded to float32 ONCE into the workspace: the correctly rounded cosine.  (Unit rows rounded to float32
//                first leave c[i][i] = 1 +- 2^-24 for a sequence against itself, and a term in its gradient that nothing
//                cancels; measured at 200 times the error of a numpy float32 evaluation whose c[i][i] happened to be 1.)
//             3. wave 0 alone, the dependent sweep: rows on lanes in bands of 64, lane i at column s - i of anti-diagonal s,
//                the row above over a DPP wave shift (shr1_f64), the band's last row handed on through LDS;
//                r = (1 - c) + softmin(diag, up, left) about the minimum, in float64; r goes to the workspace (keep) as
//                float64.  The cells a lane needs are fetched SQ_CH steps ahead of the chain.
//   backward  1. wave 0 alone, the sweep the other way (bands last to first, the row BELOW over wave_shl:1, the band's first
//                row handed up through LDS): with q = r - d (a cell's softmin), E[i][j] = sum over its three successors (a, b)
//                of E[a][b] exp((q[a][b] - r[i][j]) / gamma).  The three weights depend on r alone, so only three float64
//                multiply-adds are on the dependent chain.  E goes to the workspace as float64.
//             2. all four waves: the rows' and columns' sums of E c, then g1[i][k] = -(w / |x_i|) (sum_j E[i][j] y^_j[k] -
//                (sum_j E[i][j] c[i][j]) x^_i[k]) (a row below the clamp: -(w 1e6) sum_j E[i][j] y^_j[k]) and g2 alike, a
//                thread per element, j (i) ascending, float64 with x^ = x / max(|x|, 1e-6) formed in float64, rounded once.
// No atomics; every sum has one order that depends on the problem alone; a problem's addresses in the workspace depend on
// its position, its arithmetic does not.  Every word of the workspace that is read was written by the same call (forward) or by
// the forward the header vouches for (backward).
#include "common.h"
#include "dtw_wave.h"
#include "../../include/abnet3_hip_next.h"

#include <math.h>
#include <stdlib.h>

#include <vector>

namespace abn {

constexpr int SQ_MAX_LEN = 256;             // rows of either side: the LDS boundary row and the row / column sums
constexpr int SQ_MAX_D = 1024;
constexpr int64_t SQ_MAX_P = 1 << 24;
constexpr int SQ_T = 256;                   // threads of a workgroup
constexpr int SQ_CH = 8;                    // steps of the sweep whose cells are in registers ahead of the chain
constexpr int SQ_MAX_GRID = 2048;           // workgroups: four are resident per CU (registers), the rest queue behind them
constexpr double SQ_EPS = 1e-6;
constexpr uint64_t SQ_MAGIC = 0x7164747764666f73ull;

struct SqHeader {                           // the first 64 bytes of the workspace: what the last forward on it was
    uint64_t magic;
    int64_t P, R, N1, N2, cells;
    int32_t D, keep;
    float gamma;
    uint32_t hash;                          // of off1, n1, off2, n2 and e's address (sq_hash)
};
static_assert(sizeof(SqHeader) == 64, "the header is 64 bytes");

struct SqLayout { int64_t pre, nrm, C, Rr, E, bytes; };
static SqLayout sq_layout(int64_t P, int64_t N1, int64_t N2, int64_t cells, int64_t D, int keep)
{
    SqLayout l;
    (void)D;                                                // (nothing in the workspace is D wide: the rows are read from e)
    int64_t o = sizeof(SqHeader);
    l.pre = o; o += align_up(3 * (P + 1) * 8, 16);          // exclusive prefix sums of n1, n2, n1 * n2
    l.nrm = o; o += (N1 + N2) * 16;                         // per row: 1 / max(|x|, eps), |x| (float64)
    l.C = o; o += align_up(cells * 4, 16);                  // c, float32, [n][m] a problem
    l.Rr = o; if (keep) o += cells * 8;                     // r, float64
    l.E = o; if (keep) o += cells * 8;                      // E, float64 (written by the backward)
    l.bytes = o;
    return l;
}

struct SqP {
    const float* e; const int64_t* off1; const int32_t* n1; const int64_t* off2; const int32_t* n2;
    int64_t P, N1;
    int D, keep;
    double gamma, inv_gamma;
    SqHeader hdr;
    SqHeader* hdr_out;
    int64_t* pre; double* nrm; float* C; double* Rr; double* E;
    float* value; const float* w; float* g1; float* g2;
};

// lane l receives lane l + 1's value (lane 63: overridden by the caller)
__device__ __forceinline__ double shl1_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);      // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// The four dot products of rows x0, x1 against y0, y1 (dtw_wave.h's 2 x 2 tile: four chains share their loads), each a float64
// fma chain in k order over the RAW float32 rows: a product of two floats is exact in float64, so the chain is the dot product
// to D 2^-53.  VEC (D % 4 == 0 and a 16-byte aligned table, the same for every problem of a call) only widens the loads: the
// operations and their order are the same, so are the bits.
template <bool VEC>
__device__ __forceinline__ void sq_dot_tile(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ y0,
                                            const float* __restrict__ y1, int D, double (&acc)[4])
{
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    if (VEC) {
        for (int k = 0; k < D; k += 4) {
            const float4 p = *reinterpret_cast<const float4*>(x0 + k), q = *reinterpret_cast<const float4*>(x1 + k);
            const float4 u = *reinterpret_cast<const float4*>(y0 + k), v = *reinterpret_cast<const float4*>(y1 + k);
            const double pd[4] = {p.x, p.y, p.z, p.w}, qd[4] = {q.x, q.y, q.z, q.w}, ud[4] = {u.x, u.y, u.z, u.w}, vd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                a00 = fma(pd[c], ud[c], a00); a01 = fma(pd[c], vd[c], a01); a10 = fma(qd[c], ud[c], a10); a11 = fma(qd[c], vd[c], a11);
            }
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const double pd = x0[k], qd = x1[k], ud = y0[k], vd = y1[k];
            a00 = fma(pd, ud, a00); a01 = fma(pd, vd, a01); a10 = fma(qd, ud, a10); a11 = fma(qd, vd, a11);
        }
    }
    acc[0] = a00; acc[1] = a01; acc[2] = a10; acc[3] = a11;
}

// One workgroup: the three exclusive prefix sums over the problems, and the header.
__global__ __launch_bounds__(SQ_T) void sq_scan_kernel(SqP p)
{
    __shared__ int64_t sh[3][SQ_T];
    const int t = threadIdx.x;
    const int64_t per = (p.P + SQ_T - 1) / SQ_T;
    const int64_t b = min(p.P, (int64_t)t * per), e = min(p.P, b + per);
    int64_t a0 = 0, a1 = 0, a2 = 0;
    for (int64_t q = b; q < e; ++q) {
        const int64_t n = p.n1[q], m = p.n2[q];
        a0 += n; a1 += m; a2 += n * m;
    }
    sh[0][t] = a0; sh[1][t] = a1; sh[2][t] = a2;
    __syncthreads();
    for (int o = 1; o < SQ_T; o <<= 1) {
        const int64_t v0 = t >= o ? sh[0][t - o] : 0, v1 = t >= o ? sh[1][t - o] : 0, v2 = t >= o ? sh[2][t - o] : 0;
        __syncthreads();
        sh[0][t] += v0; sh[1][t] += v1; sh[2][t] += v2;
        __syncthreads();
    }
    int64_t x0 = sh[0][t] - a0, x1 = sh[1][t] - a1, x2 = sh[2][t] - a2;
    const int64_t s = p.P + 1;
    for (int64_t q = b; q < e; ++q) {
        const int64_t n = p.n1[q], m = p.n2[q];
        p.pre[q] = x0; p.pre[s + q] = x1; p.pre[2 * s + q] = x2;
        x0 += n; x1 += m; x2 += n * m;
    }
    if (t == SQ_T - 1) { p.pre[p.P] = sh[0][t]; p.pre[s + p.P] = sh[1][t]; p.pre[2 * s + p.P] = sh[2][t]; }
    if (t == 0) {
        SqHeader* const h = p.hdr_out;
        h->magic = p.hdr.magic; h->P = p.hdr.P; h->R = p.hdr.R; h->N1 = p.hdr.N1; h->N2 = p.hdr.N2; h->cells = p.hdr.cells;
        h->D = p.hdr.D; h->keep = p.hdr.keep; h->gamma = p.hdr.gamma; h->hash = p.hdr.hash;
    }
}

template <bool VEC>
__global__ __launch_bounds__(SQ_T) void sq_forward_kernel(SqP p)
{
    __shared__ double bnd[SQ_MAX_LEN];          // the band's last row, per column
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double INF = __builtin_inf();
    const int D = p.D;
    for (int64_t q = blockIdx.x; q < p.P; q += gridDim.x) {
        const int n = p.n1[q], m = p.n2[q];
        const int64_t r1 = p.pre[q], r2 = p.N1 + p.pre[(p.P + 1) + q], c0 = p.pre[2 * (p.P + 1) + q];
        const float* const X = p.e + p.off1[q] * D;
        const float* const Y = p.e + p.off2[q] * D;
        float* const Cc = p.C + c0;
        double* const nr1 = p.nrm + 2 * r1;
        double* const nr2 = p.nrm + 2 * r2;
        // ---- 1. the norms: a wave per row
        for (int row = wave; row < n + m; row += SQ_T / 64) {
            const bool s2 = row >= n;
            const float* const src = s2 ? Y + (int64_t)(row - n) * D : X + (int64_t)row * D;
            double ss = 0.0;
            for (int k = lane; k < D; k += 64) ss = fma((double)src[k], (double)src[k], ss);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
            const double nrm = sqrt(ss);
            if (lane == 0) {
                double* const o = s2 ? nr2 + 2 * (row - n) : nr1 + 2 * row;
                o[0] = 1.0 / fmax(nrm, SQ_EPS);
                o[1] = nrm;
            }
        }
        __syncthreads();
        // ---- 2. the cells, 2 x 2 tiles (an odd last row / column repeats its neighbour: the same value stored twice)
        {
            const int tc = (m + 1) >> 1, ntile = ((n + 1) >> 1) * tc;
            for (int tt = t; tt < ntile; tt += SQ_T) {
                const int ti = tt / tc, tj = tt - ti * tc;
                const int ia = 2 * ti, ib = min(ia + 1, n - 1), ja = 2 * tj, jb = min(ja + 1, m - 1);
                double acc[4];
                sq_dot_tile<VEC>(X + (int64_t)ia * D, X + (int64_t)ib * D, Y + (int64_t)ja * D, Y + (int64_t)jb * D, D, acc);
                const double xa = nr1[2 * ia], xb = nr1[2 * ib], ya = nr2[2 * ja], yb = nr2[2 * jb];
                Cc[(int64_t)ia * m + ja] = (float)(acc[0] * xa * ya);
                Cc[(int64_t)ia * m + jb] = (float)(acc[1] * xa * yb);
                Cc[(int64_t)ib * m + ja] = (float)(acc[2] * xb * ya);
                Cc[(int64_t)ib * m + jb] = (float)(acc[3] * xb * yb);
            }
        }
        __syncthreads();
        // ---- 3. the sweep
        if (wave == 0) {
            double fin = 0.0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int nr = min(64, n - i0);
                const bool feed = i0 + 64 < n, has_up = i0 > 0, live = lane < nr;
                const float* const crow = Cc + (int64_t)(i0 + (live ? lane : 0)) * m;
                double* const rrow = p.Rr + c0 + (int64_t)(i0 + (live ? lane : 0)) * m;
                double p1 = INF, up_prev = (i0 == 0 && lane == 0) ? 0.0 : INF;
                const int ndiag = nr + m - 1;
                float cur[SQ_CH], nxt[SQ_CH];
#pragma unroll
                for (int e = 0; e < SQ_CH; ++e) {
                    const int j = e - lane;
                    cur[e] = (live && (unsigned)j < (unsigned)m) ? crow[j] : 0.0f;
                }
                for (int s0 = 0; s0 < ndiag; s0 += SQ_CH) {
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) {
                        const int j = s0 + SQ_CH + e - lane;
                        nxt[e] = (live && (unsigned)j < (unsigned)m) ? crow[j] : 0.0f;
                    }
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) {
                        const int s = s0 + e, j = s - lane;
                        if (s < ndiag) {
                            double up = shr1_f64(p1);
                            if (lane == 0) up = (has_up && s < m) ? bnd[s] : INF;
                            const double dg = up_prev, left = p1;
                            up_prev = up;
                            if (live && (unsigned)j < (unsigned)m) {
                                const double mn = fmin(dg, fmin(up, left));
                                const double sum = exp((mn - dg) * p.inv_gamma) + exp((mn - up) * p.inv_gamma) +
                                                   exp((mn - left) * p.inv_gamma);
                                const float d = 1.0f - cur[e];
                                p1 = (double)d + (mn - p.gamma * log(sum));
                                if (p.keep) rrow[j] = p1;
                                if (feed && lane == 63) bnd[j] = p1;
                            }
                        }
                    }
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) cur[e] = nxt[e];
                }
                if (i0 + nr == n) fin = __shfl(p1, nr - 1);
                wave_lds_sync();
            }
            if (lane == 0) p.value[q] = (float)fin;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SQ_T) void sq_backward_kernel(SqP p)
{
    __shared__ double bE[SQ_MAX_LEN], bQ[SQ_MAX_LEN];       // the band's first row, per column: E and q = r - d
    __shared__ double sc1[SQ_MAX_LEN], sc2[SQ_MAX_LEN];     // sum_j E c of a row, sum_i E c of a column
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double INF = __builtin_inf();
    const int D = p.D;
    for (int64_t q = blockIdx.x; q < p.P; q += gridDim.x) {
        const int n = p.n1[q], m = p.n2[q];
        const int64_t r1 = p.pre[q], r2 = p.N1 + p.pre[(p.P + 1) + q], c0 = p.pre[2 * (p.P + 1) + q];
        const float* const X = p.e + p.off1[q] * D;
        const float* const Y = p.e + p.off2[q] * D;
        const double* const nr1 = p.nrm + 2 * r1;
        const double* const nr2 = p.nrm + 2 * r2;
        const float* const Cc = p.C + c0;
        const double* const Rr = p.Rr + c0;
        double* const Ee = p.E + c0;
        const double wq = (double)p.w[q];
        // ---- 1. the sweep, last band first
        if (wave == 0) {
            for (int i0 = ((n - 1) / 64) * 64; i0 >= 0; i0 -= 64) {
                const int nr = min(64, n - i0);
                const bool below = i0 + 64 < n, feed = i0 > 0, live = lane < nr;
                const int64_t ro = (int64_t)(i0 + (live ? lane : 0)) * m;
                const float* const crow = Cc + ro;
                const double* const rrow = Rr + ro;
                double* const erow = Ee + ro;
                const bool last_row = i0 + lane == n - 1;
                double E1 = 0.0, q1 = -INF, Edg = 0.0, qdg = -INF;      // cell (i, j + 1); cell (i + 1, j + 1)
                const int ndiag = nr + m - 1;
                float ccur[SQ_CH], cnxt[SQ_CH];
                double rcur[SQ_CH], rnxt[SQ_CH];
#pragma unroll
                for (int e = 0; e < SQ_CH; ++e) {
                    const int j = ndiag - 1 - e - lane;
                    const bool in = live && (unsigned)j < (unsigned)m;
                    ccur[e] = in ? crow[j] : 0.0f;
                    rcur[e] = in ? rrow[j] : 0.0;
                }
                for (int s0 = ndiag - 1; s0 >= 0; s0 -= SQ_CH) {
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) {
                        const int j = s0 - SQ_CH - e - lane;
                        const bool in = live && (unsigned)j < (unsigned)m;
                        cnxt[e] = in ? crow[j] : 0.0f;
                        rnxt[e] = in ? rrow[j] : 0.0;
                    }
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) {
                        const int s = s0 - e, j = s - lane;
                        if (s >= 0) {
                            double Ed = shl1_f64(E1), qd = shl1_f64(q1);
                            if (lane == 63) {
                                const bool in = below && (unsigned)j < (unsigned)m;
                                Ed = in ? bE[in ? j : 0] : 0.0;
                                qd = in ? bQ[in ? j : 0] : -INF;
                            }
                            const double Eg = Edg, qg = qdg;
                            Edg = Ed;
                            qdg = qd;
                            if (live && (unsigned)j < (unsigned)m) {
                                const double r = rcur[e];
                                const float d = 1.0f - ccur[e];
                                const double qc = r - (double)d;
                                const double wd = exp((qd - r) * p.inv_gamma), wr = exp((q1 - r) * p.inv_gamma),
                                             wg = exp((qg - r) * p.inv_gamma);
                                double Ev = fma(Eg, wg, fma(E1, wr, Ed * wd));
                                if (last_row && j == m - 1) Ev = 1.0;
                                E1 = Ev;
                                q1 = qc;
                                erow[j] = Ev;
                                if (feed && lane == 0) { bE[j] = Ev; bQ[j] = qc; }
                            }
                        }
                    }
#pragma unroll
                    for (int e = 0; e < SQ_CH; ++e) { ccur[e] = cnxt[e]; rcur[e] = rnxt[e]; }
                }
                wave_lds_sync();
            }
        }
        __syncthreads();
        // ---- 2. the sums of E c over a row (side 1) and over a column (side 2)
        for (int idx = t; idx < n + m; idx += SQ_T) {
            double a = 0.0;
            if (idx < n) {
                for (int j = 0; j < m; ++j) a = fma(Ee[(int64_t)idx * m + j], (double)Cc[(int64_t)idx * m + j], a);
                sc1[idx] = a;
            } else {
                const int j = idx - n;
                for (int i = 0; i < n; ++i) a = fma(Ee[(int64_t)i * m + j], (double)Cc[(int64_t)i * m + j], a);
                sc2[j] = a;
            }
        }
        __syncthreads();
        // ---- 3. the gradients, a thread per element
        float* const G1 = p.g1 + r1 * D;
        float* const G2 = p.g2 + (r2 - p.N1) * D;
        for (int idx = t; idx < n * D; idx += SQ_T) {
            const int i = idx / D, k = idx - i * D;
            double a = 0.0;
            for (int j = 0; j < m; ++j) a = fma(Ee[(int64_t)i * m + j], (double)Y[(int64_t)j * D + k] * nr2[2 * j], a);
            const double inv = nr1[2 * i], nrm = nr1[2 * i + 1];
            if (nrm >= SQ_EPS) a -= sc1[i] * ((double)X[(int64_t)i * D + k] * inv);
            G1[idx] = wq == 0.0 ? 0.0f : (float)(-(wq * inv) * a);
        }
        for (int idx = t; idx < m * D; idx += SQ_T) {
            const int j = idx / D, k = idx - j * D;
            double a = 0.0;
            for (int i = 0; i < n; ++i) a = fma(Ee[(int64_t)i * m + j], (double)X[(int64_t)i * D + k] * nr1[2 * i], a);
            const double inv = nr2[2 * j], nrm = nr2[2 * j + 1];
            if (nrm >= SQ_EPS) a -= sc2[j] * ((double)Y[(int64_t)j * D + k] * inv);
            G2[idx] = wq == 0.0 ? 0.0f : (float)(-(wq * inv) * a);
        }
        __syncthreads();
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
static int sq_check_scalars(const char* what, int64_t P, int64_t D)
{
    ABN_REQUIRE(P >= 0, "%s: P = %lld out of range", what, (long long)P);
    ABN_REQUIRE(D >= 1, "%s: D = %lld out of range", what, (long long)D);
    if (D > SQ_MAX_D || P > SQ_MAX_P) {
        set_error("%s: P = %lld, D = %lld, supported D <= %d (abnq_softdtw_max_d), P <= %lld", what, (long long)P, (long long)D,
                  SQ_MAX_D, (long long)SQ_MAX_P);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

static int sq_check_lengths(const char* what, const int32_t* n1, const int32_t* n2, int64_t P, int64_t* N1, int64_t* N2,
                            int64_t* cells)
{
    int64_t a = 0, b = 0, c = 0;
    for (int64_t q = 0; q < P; ++q) {
        const int64_t n = n1[q], m = n2[q];
        ABN_REQUIRE(n >= 1 && m >= 1, "%s: problem %lld has lengths %lld, %lld: an empty side", what, (long long)q, (long long)n,
                    (long long)m);
        if (n > SQ_MAX_LEN || m > SQ_MAX_LEN) {
            set_error("%s: problem %lld has lengths %lld, %lld, supported <= %d (abnq_softdtw_max_len)", what, (long long)q,
                      (long long)n, (long long)m, SQ_MAX_LEN);
            return ABN_E_UNSUPPORTED;
        }
        a += n; b += m; c += n * m;
    }
    *N1 = a; *N2 = b; *cells = c;
    return ABN_OK;
}

// The four device arrays (and, for the backward, the workspace's header) on the host: staging kept per thread (a std::vector,
// released with the thread), one wait on the stream.  The call's refusals depend on them and come before any launch.
static thread_local std::vector<char> sq_stage;

// FNV-1a over the problem table and e's address: what the header keeps of WHICH problem the forward ran on.
static uint32_t sq_hash(const void* e, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int64_t P)
{
    uint32_t h = 2166136261u;
    auto eat = [&h](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 16777619u;
    };
    const uintptr_t a = reinterpret_cast<uintptr_t>(e);
    eat(&a, sizeof a);
    eat(off1, (size_t)P * 8); eat(n1, (size_t)P * 4); eat(off2, (size_t)P * 8); eat(n2, (size_t)P * 4);
    return h;
}

static int sq_fetch(const char* what, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int64_t P,
                    const void* hdr, hipStream_t st, const int64_t** h_off1, const int32_t** h_n1, const int64_t** h_off2,
                    const int32_t** h_n2, const SqHeader** h_hdr)
{
    const size_t a8 = (size_t)align_up(P * 8, 16), a4 = (size_t)align_up(P * 4, 16), need = 64 + 2 * a8 + 2 * a4;
    try {
        if (sq_stage.size() < need) sq_stage.resize(need + need / 2);
    } catch (...) {
        set_error("%s: no host memory for the problem table (%lld bytes)", what, (long long)need);
        return ABN_E_LAUNCH;
    }
    char* const b = sq_stage.data();
    // the four arrays end to end in one allocation (off1, off2, n1, n2: how abnet3_amd/softdtw.py uploads them): one copy
    const bool packed = off2 == off1 + P && n1 == reinterpret_cast<const int32_t*>(off1 + 2 * P) && n2 == n1 + P;
    const size_t o2 = packed ? (size_t)P * 8 : a8, o3 = packed ? (size_t)P * 16 : 2 * a8, o4 = packed ? (size_t)P * 20 : 2 * a8 + a4;
    hipError_t e = hipSuccess;
    if (hdr) e = hipMemcpyAsync(b, hdr, 64, hipMemcpyDeviceToHost, st);
    if (packed) {
        if (e == hipSuccess) e = hipMemcpyAsync(b + 64, off1, (size_t)P * 24, hipMemcpyDeviceToHost, st);
    } else {
        if (e == hipSuccess) e = hipMemcpyAsync(b + 64, off1, (size_t)P * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(b + 64 + o2, off2, (size_t)P * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(b + 64 + o3, n1, (size_t)P * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(b + 64 + o4, n2, (size_t)P * 4, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("%s: reading the problem table: %s", what, hipGetErrorString(e));
        return ABN_E_LAUNCH;
    }
    *h_hdr = reinterpret_cast<const SqHeader*>(b);
    *h_off1 = reinterpret_cast<const int64_t*>(b + 64);
    *h_off2 = reinterpret_cast<const int64_t*>(b + 64 + o2);
    *h_n1 = reinterpret_cast<const int32_t*>(b + 64 + o3);
    *h_n2 = reinterpret_cast<const int32_t*>(b + 64 + o4);
    return ABN_OK;
}

static bool sq_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int sq_check_common(const char* what, const float* e, int64_t R, int64_t D, const int64_t* off1, const int32_t* n1,
                           const int64_t* off2, const int32_t* n2, int64_t P, float gamma, const void* ws, int64_t ws_bytes)
{
    const int rc = sq_check_scalars(what, P, D);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(R >= 0 && R < (1LL << 40), "%s: R = %lld out of range", what, (long long)R);
    ABN_REQUIRE(__builtin_isfinite(gamma) && gamma > 0.0f && __builtin_isfinite(1.0 / (double)gamma),
                "%s: gamma = %g must be finite and > 0", what, (double)gamma);
    ABN_REQUIRE(ws_bytes >= 0, "%s: ws_bytes = %lld out of range", what, (long long)ws_bytes);
    if (P == 0) return ABN_OK;
    ABN_REQUIRE(e && off1 && n1 && off2 && n2 && ws, "%s: null pointer", what);
    ABN_REQUIRE(sq_aligned(e, 4) && sq_aligned(off1, 8) && sq_aligned(off2, 8) && sq_aligned(n1, 4) && sq_aligned(n2, 4),
                "%s: a misaligned table (e, n1, n2: 4 bytes; off1, off2: 8 bytes)", what);
    ABN_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);
    return ABN_OK;
}

static int sq_check_offsets(const char* what, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                            int64_t P, int64_t R)
{
    for (int64_t q = 0; q < P; ++q)
        ABN_REQUIRE(off1[q] >= 0 && off2[q] >= 0 && off1[q] <= R - n1[q] && off2[q] <= R - n2[q],
                    "%s: problem %lld reads rows %lld + %d, %lld + %d of a table of %lld", what, (long long)q, (long long)off1[q],
                    (int)n1[q], (long long)off2[q], (int)n2[q], (long long)R);
    return ABN_OK;
}

static int sq_grid(int64_t P)
{
    const char* v = getenv("ABN_SDTW_GRID");        // read at every call: a test that sets it needs no reload
    int g = v ? atoi(v) : 0;
    if (g <= 0 || g > SQ_MAX_GRID) g = SQ_MAX_GRID;
    return (int)(P < g ? P : g);
}

static void sq_bind(SqP& p, void* ws, const SqLayout& l)
{
    char* const base = static_cast<char*>(ws);
    p.hdr_out = reinterpret_cast<SqHeader*>(base);
    p.pre = reinterpret_cast<int64_t*>(base + l.pre);
    p.nrm = reinterpret_cast<double*>(base + l.nrm);
    p.C = reinterpret_cast<float*>(base + l.C);
    p.Rr = reinterpret_cast<double*>(base + l.Rr);
    p.E = reinterpret_cast<double*>(base + l.E);
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abnq_softdtw_max_len(void) { return SQ_MAX_LEN; }
extern "C" int64_t abnq_softdtw_max_d(void) { return SQ_MAX_D; }

extern "C" int64_t abnq_softdtw_ws_bytes(const int32_t* n1_host, const int32_t* n2_host, int64_t P, int64_t D, int keep)
{
    if (sq_check_scalars("abnq_softdtw_ws_bytes", P, D) != ABN_OK) return -1;
    if (P > 0 && (!n1_host || !n2_host)) {
        set_error("abnq_softdtw_ws_bytes: null pointer");
        return -1;
    }
    int64_t N1 = 0, N2 = 0, cells = 0;
    if (sq_check_lengths("abnq_softdtw_ws_bytes", n1_host, n2_host, P, &N1, &N2, &cells) != ABN_OK) return -1;
    return sq_layout(P, N1, N2, cells, D, keep != 0).bytes;
}

extern "C" int abnq_softdtw_forward(const float* e, int64_t R, int64_t D, const int64_t* off1, const int32_t* n1,
                                    const int64_t* off2, const int32_t* n2, int64_t P, float gamma, float* value, void* ws,
                                    int64_t ws_bytes, int keep, void* stream)
{
    const char* const what = "abnq_softdtw_forward";
    int rc = sq_check_common(what, e, R, D, off1, n1, off2, n2, P, gamma, ws, ws_bytes);
    if (rc != ABN_OK) return rc;
    if (P == 0) return ABN_OK;
    ABN_REQUIRE(value && sq_aligned(value, 4), "%s: value is null or misaligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t *h_off1, *h_off2;
    const int32_t *h_n1, *h_n2;
    const SqHeader* h_hdr;
    rc = sq_fetch(what, off1, n1, off2, n2, P, nullptr, st, &h_off1, &h_n1, &h_off2, &h_n2, &h_hdr);
    if (rc != ABN_OK) return rc;
    int64_t N1 = 0, N2 = 0, cells = 0;
    rc = sq_check_lengths(what, h_n1, h_n2, P, &N1, &N2, &cells);
    if (rc != ABN_OK) return rc;
    rc = sq_check_offsets(what, h_off1, h_n1, h_off2, h_n2, P, R);
    if (rc != ABN_OK) return rc;
    const SqLayout l = sq_layout(P, N1, N2, cells, D, keep != 0);
    if (ws_bytes < l.bytes) {
        set_error("%s: the workspace has %lld bytes, abnq_softdtw_ws_bytes asks for %lld", what, (long long)ws_bytes, (long long)l.bytes);
        return ABN_E_WORKSPACE;
    }
    SqP p = {};
    p.e = e; p.off1 = off1; p.n1 = n1; p.off2 = off2; p.n2 = n2;
    p.P = P; p.N1 = N1; p.D = (int)D; p.keep = keep != 0;
    p.gamma = (double)gamma; p.inv_gamma = 1.0 / (double)gamma;
    p.hdr.magic = SQ_MAGIC; p.hdr.P = P; p.hdr.R = R; p.hdr.N1 = N1; p.hdr.N2 = N2; p.hdr.cells = cells;
    p.hdr.D = (int32_t)D; p.hdr.keep = keep != 0; p.hdr.gamma = gamma; p.hdr.hash = sq_hash(e, h_off1, h_n1, h_off2, h_n2, P);
    sq_bind(p, ws, l);
    p.value = value;
    hipLaunchKernelGGL(sq_scan_kernel, dim3(1), dim3(SQ_T), 0, st, p);
    ABN_CHECK_LAUNCH("abnq_softdtw_forward (prefix sums)");
    if (D % 4 == 0 && aligned16(e)) hipLaunchKernelGGL(sq_forward_kernel<true>, dim3((unsigned)sq_grid(P)), dim3(SQ_T), 0, st, p);
    else hipLaunchKernelGGL(sq_forward_kernel<false>, dim3((unsigned)sq_grid(P)), dim3(SQ_T), 0, st, p);
    ABN_CHECK_LAUNCH("abnq_softdtw_forward");
    return ABN_OK;
}

extern "C" int abnq_softdtw_backward(const float* e, int64_t R, int64_t D, const int64_t* off1, const int32_t* n1,
                                     const int64_t* off2, const int32_t* n2, int64_t P, float gamma, const float* w, float* g1,
                                     float* g2, void* ws, int64_t ws_bytes, void* stream)
{
    const char* const what = "abnq_softdtw_backward";
    int rc = sq_check_common(what, e, R, D, off1, n1, off2, n2, P, gamma, ws, ws_bytes);
    if (rc != ABN_OK) return rc;
    if (P == 0) return ABN_OK;
    ABN_REQUIRE(w && g1 && g2, "%s: null pointer", what);
    ABN_REQUIRE(sq_aligned(w, 4) && sq_aligned(g1, 4) && sq_aligned(g2, 4), "%s: a misaligned table (w, g1, g2: 4 bytes)", what);
    ABN_REQUIRE(ws_bytes >= (int64_t)sizeof(SqHeader), "%s: the workspace has %lld bytes, less than its header", what,
                (long long)ws_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t *h_off1, *h_off2;
    const int32_t *h_n1, *h_n2;
    const SqHeader* h_hdr;
    rc = sq_fetch(what, off1, n1, off2, n2, P, ws, st, &h_off1, &h_n1, &h_off2, &h_n2, &h_hdr);
    if (rc != ABN_OK) return rc;
    int64_t N1 = 0, N2 = 0, cells = 0;
    rc = sq_check_lengths(what, h_n1, h_n2, P, &N1, &N2, &cells);
    if (rc != ABN_OK) return rc;
    rc = sq_check_offsets(what, h_off1, h_n1, h_off2, h_n2, P, R);
    if (rc != ABN_OK) return rc;
    const SqLayout l = sq_layout(P, N1, N2, cells, D, 1);
    if (ws_bytes < l.bytes) {
        set_error("%s: the workspace has %lld bytes, abnq_softdtw_ws_bytes asks for %lld", what, (long long)ws_bytes, (long long)l.bytes);
        return ABN_E_WORKSPACE;
    }
    const SqHeader h = *h_hdr;
    ABN_REQUIRE(h.magic == SQ_MAGIC, "%s: no abnq_softdtw_forward has run on this workspace", what);
    ABN_REQUIRE(h.keep == 1, "%s: the forward on this workspace ran with keep = 0: nothing was stored for a backward", what);
    ABN_REQUIRE(h.P == P && h.R == R && h.D == (int32_t)D && h.N1 == N1 && h.N2 == N2 && h.cells == cells && h.gamma == gamma &&
                    h.hash == sq_hash(e, h_off1, h_n1, h_off2, h_n2, P),
                "%s: the forward on this workspace ran on another problem (P, R, D, gamma, e's address or the problem table differ)", what);
    SqP p = {};
    p.e = e; p.off1 = off1; p.n1 = n1; p.off2 = off2; p.n2 = n2;
    p.P = P; p.N1 = N1; p.D = (int)D; p.keep = 1;
    p.gamma = (double)gamma; p.inv_gamma = 1.0 / (double)gamma;
    sq_bind(p, ws, l);
    p.w = w; p.g1 = g1; p.g2 = g2;
    hipLaunchKernelGGL(sq_backward_kernel, dim3((unsigned)sq_grid(P)), dim3(SQ_T), 0, st, p);
    ABN_CHECK_LAUNCH("abnq_softdtw_backward");
    return ABN_OK;
}
