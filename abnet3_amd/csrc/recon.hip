// recon.hip -- the reconstruction loss of the correspondence autoencoder and its gradient (abnr_recon_loss).
// abnet3_amd/loss.py (CorrespondenceLoss) states the definition, tests/cae_np.py restates it, DESIGN.md section 3.4h has the
// layout, the byte count and the error derivation.
//
// t[i] = |r1[i] - target1[i]|^2 + s |r2[i] - target2[i]|^2 over the counted rows (mode 0: y[i] == 1, the targets are the
// OTHER tower's inputs; mode 1: every row, the targets are the tower's own inputs), loss = c sum t[i], gradient 2 c (r - target)
// with c = 1 or, under avg, 1 / (|R| D (1 + s)).  HBM-bound: four input tables in, two gradient tables out.
// Up to three launches, none of which waits for another workgroup and none of which the host waits for:
//   * recon_count_kernel (mode 0 with avg only -- everywhere else the host knows c): one workgroup counts the rows with
//     y == 1 (integers: any order gives the same count) and leaves c in the workspace.
//   * recon_rows_kernel: a half-wave (32 lanes) owns a row, as in pair_loss_kernel.  Lane l takes the column quads l, l + 32,
//     ... (16-byte loads where D % 4 == 0 and the pointers allow it, four 4-byte loads of the SAME columns otherwise: either
//     path adds the same squares in the same order), differences and sums in float64, the half-wave's 32 sums folded by
//     xor-shuffles, the two sides' sums added last (a + b = b + a: swapping the sides changes no bit).  t[i] goes to the
//     workspace as a float64 (0 for an uncounted row); the gradient's second read of the row is an L1 / L2 hit.
//   * recon_sum_kernel: one workgroup adds the B row terms in an order that depends on B alone (thread t takes rows t,
//     t + 1024, ...; a fixed tree over the 1024 threads) and rounds c times the sum once.
// No floating-point atomics and no ticket counter: the workspace needs no clearing, the result has the same bits from call
// to call and for any rows-per-workgroup (ABN_RECON_ROWS).
#include "common.h"
#include "../../include/abnet3_hip_next.h"

#include <stdlib.h>

namespace abn {

constexpr int RC_HALF_WAVES = 8;                 // 256 threads = 8 half-waves, a row each
constexpr int RC_ONE_WG = 1024;                  // threads of the two one-workgroup launches (count, sum)
constexpr int64_t RC_MAX_D = 16384;
constexpr int64_t RC_MAX_B = 1 << 22;
constexpr int RC_MAX_ROWS = 4096;                // ABN_RECON_ROWS: most rows one workgroup walks

struct ReconP {
    const float* r[2];          // [B][D] the reconstructions of tower 1 / tower 2
    const float* t[2];          // [B][D] what each is held against (the mode chose them)
    const void* y; int y_dtype;
    int64_t B; int D;
    int mode, sym, avg;
    int rows_per_wg;
    double c_host;              // the loss's scale where the host knows it
    double* c_dev;              // ws: the scale recon_count_kernel left (null: c_host)
    double* t64;                // ws: [B] row terms
    float* loss; float* terms; float* dr[2];
};

__device__ __forceinline__ bool recon_is_same(const void* y, int dt, int64_t i)
{
    switch (dt) {
    case 0: return static_cast<const int8_t*>(y)[i] == 1;
    case 1: return static_cast<const int32_t*>(y)[i] == 1;
    case 2: return static_cast<const int64_t*>(y)[i] == 1;
    case 3: return static_cast<const float*>(y)[i] == 1.0f;
    default: return static_cast<const double*>(y)[i] == 1.0;
    }
}

__global__ __launch_bounds__(RC_ONE_WG) void recon_count_kernel(ReconP p)
{
    __shared__ unsigned sh[RC_ONE_WG];
    unsigned n = 0;
    for (int64_t i = threadIdx.x; i < p.B; i += 4 * RC_ONE_WG) {                      // four labels' loads in flight
        bool same[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = i + (int64_t)k * RC_ONE_WG;
            same[k] = j < p.B && recon_is_same(p.y, p.y_dtype, j);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) n += same[k] ? 1u : 0u;
    }
    sh[threadIdx.x] = n;
    __syncthreads();
    for (int o = RC_ONE_WG / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.c_dev[0] = sh[0] ? 1.0 / ((double)sh[0] * (double)p.D * (p.sym ? 2.0 : 1.0)) : 0.0;
}

// columns 4 q .. 4 q + 3 of a row; past D: zeros (their differences add +0 to a sum that is never negative)
template <bool VEC>
__device__ __forceinline__ void recon_load4(const float* row, int q, int D, float (&v)[4])
{
    if constexpr (VEC) {
        const float4 u = reinterpret_cast<const float4*>(row)[q];
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 4 * q + k < D ? row[4 * q + k] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void recon_store4(float* row, int q, int D, const float (&v)[4])
{
    if constexpr (VEC) {
        reinterpret_cast<float4*>(row)[q] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < D) row[4 * q + k] = v[k];
    }
}

__device__ __forceinline__ double recon_half_wave_sum(double v)
{
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over this lane's quads of (a - b)^2, float64, quads ascending, columns ascending (explicit fma: one form on both paths)
template <bool VEC>
__device__ __forceinline__ double recon_sq_dist(const float* a, const float* b, int nq, int D, int l)
{
    double s = 0.0;
    for (int q = l; q < nq; q += 32) {
        float u[4], v[4];
        recon_load4<VEC>(a, q, D, u);
        recon_load4<VEC>(b, q, D, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)u[k] - (double)v[k];
            s = fma(d, d, s);
        }
    }
    return s;
}

// g = 2 c (a - b) rounded once, or zeros
template <bool VEC>
__device__ __forceinline__ void recon_write_grad(float* g, const float* a, const float* b, int nq, int D, int l, bool live, double c2)
{
    for (int q = l; q < nq; q += 32) {
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            float u[4], v[4];
            recon_load4<VEC>(a, q, D, u);
            recon_load4<VEC>(b, q, D, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (float)(c2 * ((double)u[k] - (double)v[k]));
        }
        recon_store4<VEC>(g, q, D, o);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void recon_rows_kernel(ReconP p)
{
    const int sub = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int64_t r1 = r0 + p.rows_per_wg < p.B ? r0 + p.rows_per_wg : p.B;
    const int D = p.D, nq = (D + 3) / 4;
    const double c2 = 2.0 * (p.c_dev ? p.c_dev[0] : p.c_host);
    for (int64_t row = r0 + sub; row < r1; row += RC_HALF_WAVES) {
        const bool counted = p.mode == 1 || recon_is_same(p.y, p.y_dtype, row);      // (the same for the whole half-wave)
        const int64_t at = row * D;
        double term = 0.0;
        if (counted) {
            const double s1 = recon_half_wave_sum(recon_sq_dist<VEC>(p.r[0] + at, p.t[0] + at, nq, D, l));
            const double s2 = p.sym ? recon_half_wave_sum(recon_sq_dist<VEC>(p.r[1] + at, p.t[1] + at, nq, D, l)) : 0.0;
            term = s1 + s2;
        }
        if (l == 0) {
            p.t64[row] = term;
            if (p.terms) p.terms[row] = (float)term;
        }
        if (p.dr[0]) {
            recon_write_grad<VEC>(p.dr[0] + at, p.r[0] + at, p.t[0] + at, nq, D, l, counted, c2);
            recon_write_grad<VEC>(p.dr[1] + at, p.r[1] + at, p.t[1] + at, nq, D, l, counted && p.sym, c2);
        }
    }
}

__global__ __launch_bounds__(RC_ONE_WG) void recon_sum_kernel(ReconP p)
{
    __shared__ double sh[RC_ONE_WG];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < p.B; i += 4 * RC_ONE_WG) {                      // four rows' loads in flight, added in row order
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = i + (int64_t)k * RC_ONE_WG;
            v[k] = j < p.B ? p.t64[j] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a += v[k];                                       // (+0 past the end: no term is negative)
    }
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = RC_ONE_WG / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.loss[0] = (float)(sh[0] * (p.c_dev ? p.c_dev[0] : p.c_host));
}

static int recon_check_sizes(int64_t B, int64_t D, const char* what)
{
    ABN_REQUIRE(B >= 1 && D >= 1, "%s: B = %lld, D = %lld out of range", what, (long long)B, (long long)D);
    if (D > RC_MAX_D || B > RC_MAX_B) {
        set_error("%s: B = %lld, D = %lld, supported D <= %lld (abnr_recon_max_d), B <= %lld", what, (long long)B, (long long)D,
                  (long long)RC_MAX_D, (long long)RC_MAX_B);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

// ABN_RECON_ROWS (1 .. 4096) forces the rows one workgroup walks, and with them the grid; it is read from the environment at
// every call (a host getenv, no kernel depends on when), so a test that sets it needs no reload.  0 / unset: a row per half-wave.
static int recon_rows_per_wg()
{
    const char* v = getenv("ABN_RECON_ROWS");
    int n = v ? atoi(v) : 0;
    if (n <= 0) n = RC_HALF_WAVES;
    return n > RC_MAX_ROWS ? RC_MAX_ROWS : n;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abnr_recon_max_d(void) { return RC_MAX_D; }

extern "C" int64_t abnr_recon_ws_bytes(int64_t B, int64_t D)
{
    if (recon_check_sizes(B, D, "abnr_recon_ws_bytes") != ABN_OK) return -1;
    return 16 + B * 8;                               // the scale, then the row terms
}

extern "C" int abnr_recon_loss(const float* r1, const float* r2, const float* x1, const float* x2, const void* y, int y_dtype,
                               int64_t B, int64_t D, int mode, int symmetric, int avg, float* loss, float* terms, float* dr1,
                               float* dr2, void* ws, void* stream)
{
    const int rc = recon_check_sizes(B, D, "abnr_recon_loss");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(mode == 0 || mode == 1, "abnr_recon_loss: mode = %d, supported 0 (correspondence), 1 (autoencoder)", mode);
    ABN_REQUIRE(r1 && r2 && x1 && x2 && loss && ws && (y || mode == 1), "abnr_recon_loss: null pointer");
    ABN_REQUIRE(y_dtype >= 0 && y_dtype <= 4, "abnr_recon_loss: y_dtype = %d, supported 0 .. 4", y_dtype);
    ABN_REQUIRE((dr1 != nullptr) == (dr2 != nullptr), "abnr_recon_loss: dr1 and dr2 go together (both null: value only)");
    ABN_REQUIRE(aligned16(ws), "abnr_recon_loss: the workspace must be 16-byte aligned");

    ReconP p;
    p.r[0] = r1; p.r[1] = r2;
    p.t[0] = mode == 0 ? x2 : x1;
    p.t[1] = mode == 0 ? x1 : x2;
    p.y = y; p.y_dtype = y_dtype; p.B = B; p.D = (int)D;
    p.mode = mode; p.sym = symmetric != 0; p.avg = avg != 0;
    p.rows_per_wg = recon_rows_per_wg();
    const bool count = mode == 0 && p.avg;
    p.c_host = (mode == 1 && p.avg) ? 1.0 / ((double)B * (double)D * (p.sym ? 2.0 : 1.0)) : 1.0;
    p.c_dev = count ? static_cast<double*>(ws) : nullptr;
    p.t64 = reinterpret_cast<double*>(static_cast<char*>(ws) + 16);
    p.loss = loss; p.terms = terms; p.dr[0] = dr1; p.dr[1] = dr2;

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count) {
        hipLaunchKernelGGL(recon_count_kernel, dim3(1), dim3(RC_ONE_WG), 0, st, p);
        ABN_CHECK_LAUNCH("abnr_recon_loss (count)");
    }
    const bool vec = D % 4 == 0 && aligned16(r1) && aligned16(r2) && aligned16(x1) && aligned16(x2) &&
                     (!dr1 || (aligned16(dr1) && aligned16(dr2)));
    const dim3 grid((unsigned)((B + p.rows_per_wg - 1) / p.rows_per_wg));
    if (vec) hipLaunchKernelGGL(recon_rows_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(recon_rows_kernel<false>, grid, dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnr_recon_loss (rows)");
    hipLaunchKernelGGL(recon_sum_kernel, dim3(1), dim3(RC_ONE_WG), 0, st, p);
    ABN_CHECK_LAUNCH("abnr_recon_loss (sum)");
    return ABN_OK;
}
