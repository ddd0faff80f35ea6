// integrate.hip -- the integration unit of MultimodalSiameseNetwork (abnet3/integration.py:71-475): the
// attention-weighted sum or concatenation of two modality embeddings, forward and backward in ONE launch each over
// all rows of both towers.
//
//   sum     out[r, c]        = fl(fl(w * x1[r, c]) + fl((1 - w) * x2[r, c]))       (d1 == d2)
//   concat  out[r, 0:d1]     = fl(w * x1[r, :]),  out[r, d1:d1 + d2] = fl((1 - w) * x2[r, :])
//
// w is 1 (the plain units: no weight), a fixed pair (w, 1 - w), a learnt scalar read from the device (1 - w in fp32),
// or the attention w[r, k] = act(fl(z1[r, k] + z2[r, k])), k = 0 (K = 1) or k = c (K = width).  The products are
// torch's operation order and the file is built without FMA contraction (build.STRICT_FP), so the fixed and scalar
// forms give the bits of the same float32 expression on a CPU.
//
// Layout: one wavefront per row, 4 rows per 256-thread workgroup, a grid that depends on the row count only (the
// learnt scalar's gradient is a fixed-order sum: per-wave fp64 partials, one per workgroup through the ticket of
// common.h, the last workgroup adds them in index order -- repeated runs give the same bits).  Rows whose widths are
// multiples of 4 and whose pointers are 16-byte aligned move as float4 (1 KiB per wave instruction); others as floats.
#include "common.h"

namespace abn {
namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_ROWS = IG_THREADS / 64;       // rows per workgroup and pass
constexpr int IG_MAX_GRID = 2048;

struct IgArgs {
    const float* x1; const float* x2; int64_t rows; int d1, d2;
    int mode, wkind, K, act;
    float wf, wcf;                 // ABN_INTEGRATE_W_FIXED
    const float* ws;               // ABN_INTEGRATE_W_SCALAR: device scalar
    const float* z1; const float* z2;     // ABN_INTEGRATE_W_ATTENTION: [rows, K] pre-activations
    float* out; float* w_out;      // forward
    const float* w;                // backward: the forward's w [rows, K]
    const float* g; float* dx1; float* dx2; float* dz; float* dw;
    double* partial; unsigned* counter;
};

__device__ __forceinline__ float ig_act(int act, float v)
{
    return act == ABN_ACT_TANH ? tanhf(v) : 1.0f / (1.0f + expf(-v));
}

__device__ __forceinline__ float ig_act_grad(int act, float w)       // act'(z) from w = act(z)
{
    return act == ABN_ACT_TANH ? 1.0f - w * w : w * (1.0f - w);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int V> struct Vec;
template <> struct Vec<1> {
    using T = float;
    static __device__ __forceinline__ float at(const T& v, int) { return v; }
    static __device__ __forceinline__ float& at(T& v, int) { return v; }
};
template <> struct Vec<4> {
    using T = float4;
    static __device__ __forceinline__ float at(const T& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
    static __device__ __forceinline__ float& at(T& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
};

// The row's weight for element c (c a multiple of V; K == width when per-feature)
template <int V>
__device__ __forceinline__ void weights_of(const IgArgs& a, int64_t r, int c, float wrow, typename Vec<V>::T& w)
{
    using VT = typename Vec<V>::T;
    if (a.wkind == ABN_INTEGRATE_W_ATTENTION && a.K > 1) {
        const VT u = *reinterpret_cast<const VT*>(a.z1 + r * a.K + c);
        const VT v = *reinterpret_cast<const VT*>(a.z2 + r * a.K + c);
#pragma unroll
        for (int i = 0; i < V; ++i) Vec<V>::at(w, i) = ig_act(a.act, Vec<V>::at(u, i) + Vec<V>::at(v, i));
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) Vec<V>::at(w, i) = wrow;
    }
}

// the row-constant weight (everything but the per-feature attention)
__device__ __forceinline__ float row_weight(const IgArgs& a, int64_t r)
{
    switch (a.wkind) {
        case ABN_INTEGRATE_W_NONE: return 1.0f;
        case ABN_INTEGRATE_W_FIXED: return a.wf;
        case ABN_INTEGRATE_W_SCALAR: return *a.ws;
        default: return a.K == 1 ? ig_act(a.act, a.z1[r] + a.z2[r]) : 0.0f;
    }
}

__device__ __forceinline__ float complement(const IgArgs& a, float w)
{
    if (a.wkind == ABN_INTEGRATE_W_NONE) return 1.0f;
    if (a.wkind == ABN_INTEGRATE_W_FIXED) return a.wcf;
    return 1.0f - w;
}

template <int V>
__global__ __launch_bounds__(IG_THREADS) void integrate_forward_kernel(IgArgs a)
{
    using VT = typename Vec<V>::T;
    const int lane = threadIdx.x & 63;
    const int dout = a.mode == ABN_INTEGRATE_SUM ? a.d1 : a.d1 + a.d2;
    for (int64_t r = (int64_t)blockIdx.x * IG_ROWS + (threadIdx.x >> 6); r < a.rows; r += (int64_t)gridDim.x * IG_ROWS) {
        const float wrow = row_weight(a, r);
        const bool per_feature = a.wkind == ABN_INTEGRATE_W_ATTENTION && a.K > 1;
        if (a.w_out && !per_feature && lane == 0) a.w_out[r] = wrow;
        const float* x1 = a.x1 + r * a.d1;
        const float* x2 = a.x2 + r * a.d2;
        float* out = a.out + r * dout;
        if (a.mode == ABN_INTEGRATE_SUM) {
            for (int c = lane * V; c < a.d1; c += 64 * V) {
                VT w, o;
                weights_of<V>(a, r, c, wrow, w);
                const VT u = *reinterpret_cast<const VT*>(x1 + c);
                const VT v = *reinterpret_cast<const VT*>(x2 + c);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float wi = Vec<V>::at(w, i);
                    const float p1 = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(u, i) : wi * Vec<V>::at(u, i);
                    const float p2 = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(v, i) : complement(a, wi) * Vec<V>::at(v, i);
                    Vec<V>::at(o, i) = p1 + p2;
                }
                *reinterpret_cast<VT*>(out + c) = o;
                if (per_feature && a.w_out) *reinterpret_cast<VT*>(a.w_out + r * a.K + c) = w;
            }
        } else {
            for (int c = lane * V; c < a.d1; c += 64 * V) {
                VT w, o;
                weights_of<V>(a, r, c, wrow, w);
                const VT u = *reinterpret_cast<const VT*>(x1 + c);
#pragma unroll
                for (int i = 0; i < V; ++i)
                    Vec<V>::at(o, i) = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(u, i) : Vec<V>::at(w, i) * Vec<V>::at(u, i);
                *reinterpret_cast<VT*>(out + c) = o;
                if (per_feature && a.w_out) *reinterpret_cast<VT*>(a.w_out + r * a.K + c) = w;
            }
            for (int c = lane * V; c < a.d2; c += 64 * V) {
                VT w, o;
                weights_of<V>(a, r, c, wrow, w);
                const VT v = *reinterpret_cast<const VT*>(x2 + c);
#pragma unroll
                for (int i = 0; i < V; ++i)
                    Vec<V>::at(o, i) = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(v, i)
                                                                       : complement(a, Vec<V>::at(w, i)) * Vec<V>::at(v, i);
                *reinterpret_cast<VT*>(out + a.d1 + c) = o;
            }
        }
    }
}

// d out / d (x1, x2, w): dx1 = g1 * w, dx2 = g2 * (1 - w), d w = g1 * x1 - g2 * x2 (g1 = g2 = g in sum mode);
// attention: dz = d w * act'(w) (K = 1: summed over the row first); learnt scalar: dw = the sum over everything.
template <int V>
__global__ __launch_bounds__(IG_THREADS) void integrate_backward_kernel(IgArgs a)
{
    using VT = typename Vec<V>::T;
    __shared__ double wave_part[IG_ROWS];
    __shared__ bool is_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool sum = a.mode == ABN_INTEGRATE_SUM;
    const int dout = sum ? a.d1 : a.d1 + a.d2;
    const bool per_feature = a.wkind == ABN_INTEGRATE_W_ATTENTION && a.K > 1;
    const bool need_dwsum = (a.wkind == ABN_INTEGRATE_W_SCALAR && a.dw) || (a.wkind == ABN_INTEGRATE_W_ATTENTION && a.K == 1 && a.dz);
    double scalar_acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * IG_ROWS + wave; r < a.rows; r += (int64_t)gridDim.x * IG_ROWS) {
        const float wrow = a.wkind == ABN_INTEGRATE_W_ATTENTION ? (per_feature ? 0.0f : a.w[r]) : row_weight(a, r);
        const float* x1 = a.x1 + r * a.d1;
        const float* x2 = a.x2 + r * a.d2;
        const float* g = a.g + r * dout;
        const float* g2 = sum ? g : g + a.d1;
        double row_acc = 0.0;
        // the part of the row both inputs share (sum: all of it; concat: the first min(d1, d2) features when both
        // are weighted by the same w[k], i.e. K == d1 == d2 or a row weight)
        const int n1 = a.d1, n2 = a.d2;
        for (int c = lane * V; c < (n1 > n2 ? n1 : n2); c += 64 * V) {
            VT w;
            if (per_feature) w = *reinterpret_cast<const VT*>(a.w + r * a.K + c);
            else {
#pragma unroll
                for (int i = 0; i < V; ++i) Vec<V>::at(w, i) = wrow;
            }
            VT t;                      // d out / d w at each feature (fp32 products, as autograd's)
#pragma unroll
            for (int i = 0; i < V; ++i) Vec<V>::at(t, i) = 0.0f;
            if (c < n1) {
                const VT gv = *reinterpret_cast<const VT*>(g + c);
                if (a.dx1) {
                    VT d;
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        Vec<V>::at(d, i) = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(gv, i) : Vec<V>::at(gv, i) * Vec<V>::at(w, i);
                    *reinterpret_cast<VT*>(a.dx1 + r * n1 + c) = d;
                }
                if (a.wkind != ABN_INTEGRATE_W_NONE && a.wkind != ABN_INTEGRATE_W_FIXED) {
                    const VT u = *reinterpret_cast<const VT*>(x1 + c);
#pragma unroll
                    for (int i = 0; i < V; ++i) Vec<V>::at(t, i) = Vec<V>::at(gv, i) * Vec<V>::at(u, i);
                }
            }
            if (c < n2) {
                const VT gv = *reinterpret_cast<const VT*>(g2 + c);
                if (a.dx2) {
                    VT d;
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        Vec<V>::at(d, i) = a.wkind == ABN_INTEGRATE_W_NONE ? Vec<V>::at(gv, i)
                                                                           : Vec<V>::at(gv, i) * complement(a, Vec<V>::at(w, i));
                    *reinterpret_cast<VT*>(a.dx2 + r * n2 + c) = d;
                }
                if (a.wkind != ABN_INTEGRATE_W_NONE && a.wkind != ABN_INTEGRATE_W_FIXED) {
                    const VT v = *reinterpret_cast<const VT*>(x2 + c);
#pragma unroll
                    for (int i = 0; i < V; ++i) Vec<V>::at(t, i) = Vec<V>::at(t, i) - Vec<V>::at(gv, i) * Vec<V>::at(v, i);
                }
            }
            if (per_feature && a.dz) {
                VT d;
#pragma unroll
                for (int i = 0; i < V; ++i) Vec<V>::at(d, i) = Vec<V>::at(t, i) * ig_act_grad(a.act, Vec<V>::at(w, i));
                *reinterpret_cast<VT*>(a.dz + r * a.K + c) = d;
            }
            if (need_dwsum) {
#pragma unroll
                for (int i = 0; i < V; ++i) row_acc += (double)Vec<V>::at(t, i);
            }
        }
        if (need_dwsum) {
            row_acc = wave_sum(row_acc);
            if (a.wkind == ABN_INTEGRATE_W_ATTENTION) {
                if (lane == 0) a.dz[r] = (float)row_acc * ig_act_grad(a.act, wrow);
            } else {
                scalar_acc += row_acc;
            }
        }
    }
    if (!(a.wkind == ABN_INTEGRATE_W_SCALAR && a.dw)) return;       // (uniform over the grid)
    if (lane == 0) wave_part[wave] = scalar_acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < IG_ROWS; ++i) s += wave_part[i];
        is_last = abn_ticket_publish(&a.partial[blockIdx.x], s, a.counter, gridDim.x);
    }
    __syncthreads();
    if (!is_last || threadIdx.x != 0) return;
    double s = 0.0;
    for (unsigned i = 0; i < gridDim.x; ++i) s += abn_ticket_partial(&a.partial[i]);
    *a.dw = (float)s;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // ready for the next call
}

int grid_of(int64_t rows)
{
    const int64_t g = (rows + IG_ROWS - 1) / IG_ROWS;
    return (int)(g < 1 ? 1 : (g > IG_MAX_GRID ? IG_MAX_GRID : g));
}

bool vec4_ok(const IgArgs& a)
{
    if (a.d1 % 4 || a.d2 % 4) return false;
    const void* ps[] = {a.x1, a.x2, a.z1, a.z2, a.out, a.w_out, a.w, a.g, a.dx1, a.dx2, a.dz};
    for (const void* p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}

int check_args(const IgArgs& a, const char* what)
{
    ABN_REQUIRE(a.rows >= 0 && a.rows < (1LL << 40), "%s: bad row count %lld", what, (long long)a.rows);
    ABN_REQUIRE(a.d1 >= 1 && a.d2 >= 1 && a.d1 < (1 << 24) && a.d2 < (1 << 24), "%s: bad widths %d, %d", what, a.d1, a.d2);
    ABN_REQUIRE(a.mode == ABN_INTEGRATE_SUM || a.mode == ABN_INTEGRATE_CONCAT, "%s: unknown mode %d", what, a.mode);
    ABN_REQUIRE(a.mode != ABN_INTEGRATE_SUM || a.d1 == a.d2, "%s: sum mode needs equal widths (%d, %d)", what, a.d1, a.d2);
    ABN_REQUIRE(a.wkind >= ABN_INTEGRATE_W_NONE && a.wkind <= ABN_INTEGRATE_W_ATTENTION, "%s: unknown weight kind %d", what, a.wkind);
    ABN_REQUIRE(a.wkind != ABN_INTEGRATE_W_SCALAR || a.ws, "%s: the learnt scalar's pointer is NULL", what);
    if (a.wkind == ABN_INTEGRATE_W_ATTENTION) {
        ABN_REQUIRE(a.act == ABN_ACT_SIGMOID || a.act == ABN_ACT_TANH, "%s: attention activation must be sigmoid or tanh", what);
        // every weight multiplies a whole row (K = 1) or one feature of both inputs (K = d1 = d2)
        ABN_REQUIRE(a.K == 1 || (a.K == a.d1 && a.K == a.d2), "%s: K = %d fits neither a row weight nor widths (%d, %d)",
                    what, a.K, a.d1, a.d2);
    }
    return ABN_OK;
}

}  // namespace
}  // namespace abn

using namespace abn;

extern "C" {

int64_t abn_integrate_ws_bytes(int64_t rows)
{
    return 8 + (int64_t)grid_of(rows < 0 ? 0 : rows) * (int64_t)sizeof(double);       // the ticket counter, then the partials
}

int abn_integrate_forward(const float* x1, int64_t d1, const float* x2, int64_t d2, int64_t rows, int mode, int weight_kind,
                          float w_fixed, float w_complement, const float* w_scalar, const float* z1, const float* z2, int64_t K,
                          int act, float* out, float* w_out, void* stream)
{
    IgArgs a = {};
    a.x1 = x1; a.x2 = x2; a.rows = rows; a.d1 = (int)d1; a.d2 = (int)d2; a.mode = mode; a.wkind = weight_kind;
    a.K = weight_kind == ABN_INTEGRATE_W_ATTENTION ? (int)K : 1; a.act = act;
    a.wf = w_fixed; a.wcf = w_complement; a.ws = w_scalar; a.z1 = z1; a.z2 = z2; a.out = out; a.w_out = w_out;
    ABN_REQUIRE(d1 >= 1 && d2 >= 1 && d1 < (1 << 24) && d2 < (1 << 24), "integrate_forward: bad widths");
    if (int rc = check_args(a, "integrate_forward")) return rc;
    if (rows == 0) return ABN_OK;
    ABN_REQUIRE(x1 && x2 && out, "integrate_forward: null pointer");
    ABN_REQUIRE(weight_kind != ABN_INTEGRATE_W_ATTENTION || (z1 && z2), "integrate_forward: attention needs z1 and z2");
    if (vec4_ok(a))
        hipLaunchKernelGGL(integrate_forward_kernel<4>, dim3(grid_of(rows)), dim3(IG_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(integrate_forward_kernel<1>, dim3(grid_of(rows)), dim3(IG_THREADS), 0, (hipStream_t)stream, a);
    ABN_CHECK_LAUNCH("integrate_forward");
    return ABN_OK;
}

int abn_integrate_backward(const float* x1, int64_t d1, const float* x2, int64_t d2, int64_t rows, int mode, int weight_kind,
                           float w_fixed, float w_complement, const float* w_scalar, const float* w, int64_t K, int act,
                           const float* g, float* dx1, float* dx2, float* dz, float* dw, void* ws, void* stream)
{
    IgArgs a = {};
    a.x1 = x1; a.x2 = x2; a.rows = rows; a.d1 = (int)d1; a.d2 = (int)d2; a.mode = mode; a.wkind = weight_kind;
    a.K = weight_kind == ABN_INTEGRATE_W_ATTENTION ? (int)K : 1; a.act = act;
    a.wf = w_fixed; a.wcf = w_complement; a.ws = w_scalar; a.w = w; a.g = g; a.dx1 = dx1; a.dx2 = dx2; a.dz = dz; a.dw = dw;
    ABN_REQUIRE(d1 >= 1 && d2 >= 1 && d1 < (1 << 24) && d2 < (1 << 24), "integrate_backward: bad widths");
    if (int rc = check_args(a, "integrate_backward")) return rc;
    if (weight_kind != ABN_INTEGRATE_W_SCALAR) a.dw = nullptr;
    if (weight_kind != ABN_INTEGRATE_W_ATTENTION) a.dz = nullptr;
    if (rows == 0) {
        if (a.dw) {
            hipMemsetAsync(a.dw, 0, sizeof(float), (hipStream_t)stream);      // an empty sum
            ABN_CHECK_LAUNCH("integrate_backward");
        }
        return ABN_OK;
    }
    ABN_REQUIRE(x1 && x2 && g, "integrate_backward: null pointer");
    ABN_REQUIRE(weight_kind != ABN_INTEGRATE_W_ATTENTION || w, "integrate_backward: attention needs the forward's w");
    ABN_REQUIRE(!a.dw || ws, "integrate_backward: the learnt scalar's gradient needs the workspace");
    a.counter = (unsigned*)ws;
    a.partial = (double*)((char*)ws + 8);
    if (vec4_ok(a))
        hipLaunchKernelGGL(integrate_backward_kernel<4>, dim3(grid_of(rows)), dim3(IG_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(integrate_backward_kernel<1>, dim3(grid_of(rows)), dim3(IG_THREADS), 0, (hipStream_t)stream, a);
    ABN_CHECK_LAUNCH("integrate_backward");
    return ABN_OK;
}

}  // extern "C"
