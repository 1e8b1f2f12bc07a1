// hispmv_krylov_multi.hip -- the vector kernels of the multi-right-hand-side Krylov entries (hispmv_krylov_multi.h; include/hispmv.h:
// hispmv_dot_multi_device, hispmv_cg_multi_device, hispmv_bicgstab_multi_device): the kernels of hispmv_krylov.hip over the columns of
// feature-major operands [n, ld].  LANES GO ACROSS COLUMNS: a thread owns 4 consecutive columns (one 16-, two 8- or four 4-byte
// accesses per row, decided per operand by its alignment and ld, same bits) and a workgroup of 256 threads owns one chunk of 1024 rows
// of one column tile of TW = 4 * CL columns, CL = 1, 2, 4, 8 or 16 column lanes.  The other RL = 256 / CL lanes go down the rows.
//
// THE ORDER OF A COLUMN'S DOT PRODUCT is the single-vector one (include/hispmv.h).  Its tree over the 256 leaves of a chunk -- leaf t =
// rows 1024 c + 4 t + j, j ascending from +0 -- is v[t] += v[t + 128], then 64, ... 1: the node at depth d holds the leaves that agree
// in the low d bits of t.  Row lane k owns the complete subtree t = k (mod RL), the CL leaves t = k + RL i: it walks them depth first
// (leaf j of the walk is i = bitrev(j); a stack of log2 CL sums), which are the steps 128 ... RL of the tree, and the steps RL / 2 ... 1
// run over the row lanes, through LDS and wavefront shuffles.  The sum over the G <= 1024 partials of a column is the same tree with leaf t = partials
// 4 t .. 4 t + 3, and every workgroup sums the partials of ITS columns itself: no finish launch, no atomics, no tickets, no waiting.
//
// PER COLUMN: a scalar block (KrylovScalar) with its own done and breakdown.  One thread per column runs the scalar rule the
// single-vector kernel runs (hispmv_krylov_scalar.h); a frozen column's updates are no-ops and its loads are skipped where all 4 columns of a thread are frozen.
// Vector arithmetic is fp32 and unfused (-ffp-contract=off), scalars are fp64 rounded once.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "hispmv_krylov_multi.h"
#include "hispmv_krylov_scalar.h"

namespace hispmv {
namespace {

// the widest access every row of an operand [n, ld] at p allows a lane of 4 columns: 4, 2 or 1 floats
__device__ __forceinline__ int width_of(const void* p, int64_t ld) {
    const uintptr_t u = (uintptr_t)p;
    return ((u & 15) == 0 && (ld & 3) == 0) ? 4 : ((u & 7) == 0 && (ld & 1) == 0) ? 2 : 1;
}
// v[0 .. nc) = p[off .. off + nc), the rest +0; w = width_of(p, ld), off = row * ld + the lane's first column
__device__ __forceinline__ void ldv(const float* p, int64_t off, int w, int nc, float v[4]) {
    if (nc == 4 && w == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p + off);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else if (nc == 4 && w == 2) {
        const float2 f = *reinterpret_cast<const float2*>(p + off), g = *reinterpret_cast<const float2*>(p + off + 2);
        v[0] = f.x; v[1] = f.y; v[2] = g.x; v[3] = g.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nc ? p[off + j] : 0.0f;
    }
}
__device__ __forceinline__ void stv(float* p, int64_t off, int w, int nc, const float v[4]) {
    if (nc == 4 && w == 4) {
        *reinterpret_cast<float4*>(p + off) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (nc == 4 && w == 2) {
        *reinterpret_cast<float2*>(p + off) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(p + off + 2) = make_float2(v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nc) p[off + j] = v[j];
    }
}
// the workspace's vectors: ldw is a multiple of 4 and they are 16-byte aligned, pad columns included
__device__ __forceinline__ void ldw4(const float* p, int64_t off, float v[4]) { ldv(p, off, 4, 4, v); }
__device__ __forceinline__ void stw4(float* p, int64_t off, const float v[4]) { stv(p, off, 4, 4, v); }

struct Shared {
    double sum[3 * 4 * kKrylovThreads];          // up to 3 sums x 256 threads x 4 columns; the results end up at thread k = 0
    float f1[kKrylovMultiTile], f2[kKrylovMultiTile];
    int act[kKrylovMultiTile], frz[kKrylovMultiTile];
};

template <int CLB>
struct Geo {
    static constexpr int CL = 1 << CLB, RL = kKrylovThreads >> CLB, TW = 4 * CL;
    int tid, cl, k, col0, col;
    bool in;          // the lane's 4 columns lie inside the workspace's leading dimension
    __device__ __forceinline__ explicit Geo(int64_t ldw) {
        tid = threadIdx.x; cl = tid & (CL - 1); k = tid >> CLB;
        col0 = blockIdx.y * TW; col = col0 + 4 * cl;
        in = col < ldw;
    }
    // leaf t of step j of the lane's depth-first walk
    __device__ __forceinline__ int leaf(int j) const { return k + RL * (CLB ? (int)(__brev((unsigned)j) >> (32 - (CLB ? CLB : 1))) : 0); }
    // where the finished sum d of local column lc lies in Shared::sum
    __device__ static __forceinline__ int at(int d, int lc) { return (d * kKrylovThreads + (lc >> 2)) * 4 + (lc & 3); }
};

// out = the sum over the lane's subtree: leaf(t, cur) adds leaf t into cur (N doubles, +0 on entry)
template <int CLB, int N, class Leaf>
__device__ __forceinline__ void subtree(const Geo<CLB>& g, Leaf&& leaf, double out[N]) {
    double st[CLB ? CLB : 1][N];
    for (int j = 0; j < Geo<CLB>::CL; ++j) {
        double cur[N];
#pragma unroll
        for (int i = 0; i < N; ++i) cur[i] = 0.0;
        leaf(g.leaf(j), cur);
        bool carry = true;
#pragma unroll
        for (int l = 0; l < CLB; ++l) {
            if (!carry) continue;
            if ((j >> l) & 1) {
#pragma unroll
                for (int i = 0; i < N; ++i) cur[i] = st[l][i] + cur[i];
            } else {
#pragma unroll
                for (int i = 0; i < N; ++i) st[l][i] = cur[i];
                carry = false;
            }
        }
        if (carry) {
#pragma unroll
            for (int i = 0; i < N; ++i) out[i] = cur[i];
        }
    }
}

// The steps RL / 2 ... 1 of the tree over the row lanes: row lane k and k + h are threads tid and tid + h * CL, so the steps are the
// thread distances 128 and 64 through LDS and 32 ... CL inside the first wavefront.  Afterwards the thread with k = 0 holds the sums
// in val and in sum[at(d, .)].
template <int CLB, int D>
__device__ __forceinline__ void block_reduce(const Geo<CLB>& g, double val[4 * D], double* sum) {
#pragma unroll
    for (int i = 0; i < 4 * D; ++i) sum[((i >> 2) * kKrylovThreads + g.tid) * 4 + (i & 3)] = val[i];
#pragma unroll
    for (int off = kKrylovThreads / 2; off >= 64; off >>= 1) {
        __syncthreads();
        if (g.tid < off) {
#pragma unroll
            for (int i = 0; i < 4 * D; ++i) {
                val[i] += sum[((i >> 2) * kKrylovThreads + g.tid + off) * 4 + (i & 3)];
                if (off > 64) sum[((i >> 2) * kKrylovThreads + g.tid) * 4 + (i & 3)] = val[i];
            }
        }
    }
    if (g.tid < 64) {
#pragma unroll
        for (int off = 32; off >= Geo<CLB>::CL; off >>= 1) {
#pragma unroll
            for (int i = 0; i < 4 * D; ++i) val[i] += __shfl_down(val[i], off, 64);
        }
        if (g.k == 0) {
#pragma unroll
            for (int i = 0; i < 4 * D; ++i) sum[((i >> 2) * kKrylovThreads + g.tid) * 4 + (i & 3)] = val[i];
        }
    }
    __syncthreads();
}

// sum[at(d, lc)] = the sum of the partials of slots[d], d < nslots, of local column lc; want: the lane needs its columns' sums
template <int CLB, int D>
__device__ __forceinline__ void sum_partials(const Geo<CLB>& g, const double* parts, int64_t groups, int64_t ldw, const int (&slots)[D], int nslots, bool want,
                                             double* sum) {
    double tot[4 * D];
#pragma unroll
    for (int i = 0; i < 4 * D; ++i) tot[i] = 0.0;
    if (want && g.in) {
        subtree<CLB, 4 * D>(g, [&](int t, double* cur) {
            if (4 * (int64_t)t >= groups) return;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int64_t gi = 4 * (int64_t)t + jj;
                if (gi >= groups) continue;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (d >= nslots) continue;
                    const double* src = parts + ((int64_t)slots[d] * groups + gi) * ldw + g.col;
#pragma unroll
                    for (int j = 0; j < 4; ++j) cur[4 * d + j] += src[j];
                }
            }
        }, tot);
    }
    block_reduce<CLB, D>(g, tot, sum);
}

// the partials of chunk blockIdx.x: the thread with k = 0 holds them
template <int CLB>
__device__ __forceinline__ void write_partial(const Geo<CLB>& g, double* parts, int64_t groups, int64_t ldw, int slot, const double* val) {
    if (g.k != 0 || !g.in) return;
    double* dst = parts + ((int64_t)slot * groups + blockIdx.x) * ldw + g.col;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = val[j];
}

// lm[j] = column j of the lane is not frozen on entry; returns whether any column of the whole tile is.  Also the defaults of the
// control words a scalar thread does not set (columns at or beyond m).
template <int CLB>
__device__ __forceinline__ bool load_frozen(const Geo<CLB>& g, const KrylovMultiStep& K, Shared& sh, bool lm[4]) {
    if (g.tid < Geo<CLB>::TW) {
        const int c = g.col0 + g.tid;
        sh.frz[g.tid] = c < K.m ? frozen(K.s_in + (int64_t)c * kKrylovState) : 1;
        sh.act[g.tid] = 0; sh.f1[g.tid] = 0.0f; sh.f2[g.tid] = 0.0f;
    }
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lm[j] = !sh.frz[4 * g.cl + j]; any |= lm[j]; }
    return any;
}
// One thread per column of the tile: f(lc, S) on the column's scalar block, which chunk 0 stores to s_out.  Ends in a barrier.
template <int CLB, class F>
__device__ __forceinline__ void scalar_phase(const Geo<CLB>& g, const KrylovMultiStep& K, F&& f) {
    const int c = g.col0 + g.tid;
    if (g.tid < Geo<CLB>::TW && c < K.m) {
        double S[kKrylovState];
#pragma unroll
        for (int i = 0; i < kKrylovState; ++i) S[i] = K.s_in ? K.s_in[(int64_t)c * kKrylovState + i] : 0.0;
        f(g.tid, S);
        if (blockIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < kKrylovState; ++i) K.s_out[(int64_t)c * kKrylovState + i] = S[i];
        }
    }
    __syncthreads();
}

// f(row, off) for the rows of leaf t that lie below n; off = row * ldw + the lane's first column
template <int CLB, class F>
__device__ __forceinline__ void leaf_rows(const Geo<CLB>& g, const KrylovMultiStep& K, int t, F&& f) {
    const int64_t row0 = (int64_t)blockIdx.x * kKrylovChunk + 4 * t;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t row = row0 + rr;
        if (row < K.n) f(row, row * K.ldw + g.col);
    }
}
__device__ __forceinline__ void add_dot(double* acc, const float a[4], const float b[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += (double)a[j] * (double)b[j];
}
// columns of the caller's x the lane may touch
template <int CLB>
__device__ __forceinline__ int cols_of(const Geo<CLB>& g, int m) { return m - g.col >= 4 ? 4 : m - g.col > 0 ? m - g.col : 0; }

template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_dot_kernel(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t n, int m, int64_t ldw, double* part) {
    __shared__ Shared sh;
    const Geo<CLB> g(ldw);
    const int nc = cols_of(g, m), wa = width_of(a, ld_a), wb = width_of(b, ld_b);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (nc > 0) {
        subtree<CLB, 4>(g, [&](int t, double* cur) {
            const int64_t row0 = (int64_t)blockIdx.x * kKrylovChunk + 4 * t;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int64_t row = row0 + rr;
                if (row >= n) continue;
                float va[4], vb[4];
                ldv(a, row * ld_a + g.col, wa, nc, va);
                ldv(b, row * ld_b + g.col, wb, nc, vb);
                add_dot(cur, va, vb);
            }
        }, acc);
    }
    block_reduce<CLB, 1>(g, acc, sh.sum);
    write_partial(g, part, gridDim.x, ldw, 0, acc);
}

template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_dot_finish_kernel(const double* part, int64_t groups, int m, int64_t ldw, double* out) {
    __shared__ Shared sh;
    const Geo<CLB> g(ldw);
    const int slots[1] = {0};
    sum_partials<CLB, 1>(g, part, groups, ldw, slots, 1, true, sh.sum);
    const int c = g.col0 + g.tid;
    if (g.tid < Geo<CLB>::TW && c < m) out[c] = sh.sum[Geo<CLB>::at(0, g.tid)];
}

// The first kernel of a solve, behind the product that gives the residuals: every column's scalar block from nothing.
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_init_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    if (g.tid < Geo<CLB>::TW) sh.act[g.tid] = 0;
    const int slots[1] = {kSlotB2};
    sum_partials<CLB, 1>(g, K.parts, K.groups, K.ldw, slots, 1, true, sh.sum);
    K.s_in = nullptr;
    scalar_phase(g, K, [&](int lc, double* S) {
        const double b2 = sh.sum[Geo<CLB>::at(0, lc)];
        krylov_rule_init(S, b2, b2, K.products, sh.act[lc]);
    });
    bool zx[4], any_zx = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) { zx[j] = sh.act[4 * g.cl + j] != 0; any_zx |= zx[j]; }
    const int nc = cols_of(g, K.m), wx = width_of(K.x, K.ld_x);
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
    if (g.in) {
        subtree<CLB, 8>(g, [&](int t, double* cur) {
            leaf_rows(g, K, t, [&](int64_t row, int64_t off) {
                float r[4], z[4];
                ldw4(K.r, off, r);
                if (K.minv) {
                    const float d = K.minv[row];
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = d * r[j];
                    add_dot(cur + 4, r, z);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = r[j];
                }
                add_dot(cur, r, r);
                stw4(K.p, off, z);
                if (K.rhat) stw4(K.rhat, off, r);
                if (any_zx) {
                    float x[4];
                    ldv(K.x, row * K.ld_x + g.col, wx, nc, x);
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = zx[j] ? 0.0f : x[j];
                    stv(K.x, row * K.ld_x + g.col, wx, nc, x);
                }
            });
        }, acc);
    }
    block_reduce<CLB, 2>(g, acc, sh.sum);
    write_partial(g, K.parts, K.groups, K.ldw, kSlotRr, acc);
    if (K.minv) write_partial(g, K.parts, K.groups, K.ldw, kSlotRho, acc + 4);
}

// a tile whose columns are all frozen: the scalar blocks move on unchanged
template <int CLB>
__device__ __forceinline__ void pass_on(const Geo<CLB>& g, const KrylovMultiStep& K) {
    scalar_phase(g, K, [](int, double*) {});
}

// The dot pass behind a product.  first: rr and rho of the initial residual still lie in their partials.
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_step_dot_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const bool same = K.slot_rho == kSlotRr;
    if (K.first) {
        const int slots[2] = {kSlotRr, K.slot_rho};
        sum_partials<CLB, 2>(g, K.parts, K.groups, K.ldw, slots, same ? 1 : 2, any, sh.sum);
    }
    scalar_phase(g, K, [&](int lc, double* S) {
        if (!K.first || frozen(S)) return;
        const double rr = sh.sum[Geo<CLB>::at(0, lc)];
        const double rho = same ? rr : sh.sum[Geo<CLB>::at(1, lc)];
        krylov_rule_first(S, rr, rho, K.tol2);
    });
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
    if (g.in && any) {
        subtree<CLB, 8>(g, [&](int t, double* cur) {
            leaf_rows(g, K, t, [&](int64_t, int64_t off) {
                float a[4], b[4];
                ldw4(K.a1, off, a);
                ldw4(K.b1, off, b);
                add_dot(cur, a, b);
                if (K.a2) {
                    ldw4(K.a2, off, a);
                    ldw4(K.b2, off, b);
                    add_dot(cur + 4, a, b);
                }
            });
        }, acc);
    }
    block_reduce<CLB, 2>(g, acc, sh.sum);
    write_partial(g, K.parts, K.groups, K.ldw, K.slot1, acc);
    if (K.a2) write_partial(g, K.parts, K.groups, K.ldw, K.slot2, acc + 4);
}

// CG: alpha = rho / (p, q); x += alpha p; r -= alpha q; the partials of (r, r) and, with minv, of (r, minv r)
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_cg_update_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const int slots[1] = {kSlotDen};
    sum_partials<CLB, 1>(g, K.parts, K.groups, K.ldw, slots, 1, any, sh.sum);
    scalar_phase(g, K, [&](int lc, double* S) {
        if (frozen(S)) return;
        const double den = sh.sum[Geo<CLB>::at(0, lc)];
        float a32;
        if (krylov_rule_alpha<false>(S, den, a32)) { sh.f1[lc] = a32; sh.act[lc] = 1; }
    });
    bool act[4], any_act = false;
    float a32[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { act[j] = sh.act[4 * g.cl + j] != 0; a32[j] = sh.f1[4 * g.cl + j]; any_act |= act[j]; }
    const int nc = cols_of(g, K.m), wx = width_of(K.x, K.ld_x);
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
    if (g.in && any_act) {
        subtree<CLB, 8>(g, [&](int t, double* cur) {
            leaf_rows(g, K, t, [&](int64_t row, int64_t off) {
                float x[4], p[4], r[4], q[4];
                const int64_t offx = row * K.ld_x + g.col;
                ldv(K.x, offx, wx, nc, x);
                ldw4(K.p, off, p);
                ldw4(K.r, off, r);
                ldw4(K.q, off, q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ap = a32[j] * p[j];
                    const float xn = x[j] + ap;
                    const float aq = a32[j] * q[j];
                    const float rn = r[j] - aq;
                    x[j] = act[j] ? xn : x[j];
                    r[j] = act[j] ? rn : r[j];
                }
                stv(K.x, offx, wx, nc, x);
                stw4(K.r, off, r);
                add_dot(cur, r, r);
                if (K.minv) {
                    const float d = K.minv[row];
                    float z[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = d * r[j];
                    add_dot(cur + 4, r, z);
                }
            });
        }, acc);
    }
    block_reduce<CLB, 2>(g, acc, sh.sum);
    if (!any_act) return;
    write_partial(g, K.parts, K.groups, K.ldw, kSlotRr, acc);
    if (K.minv) write_partial(g, K.parts, K.groups, K.ldw, kSlotRho, acc + 4);
}

// CG: the stopping rule on the new rr, then beta = rho' / rho; p = z + beta p with z = minv r (or r)
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_direction_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const bool same = K.slot_rho == kSlotRr;
    const int slots[2] = {kSlotRr, K.slot_rho};
    sum_partials<CLB, 2>(g, K.parts, K.groups, K.ldw, slots, same ? 1 : 2, any, sh.sum);
    scalar_phase(g, K, [&](int lc, double* S) {
        if (frozen(S)) return;
        const double rr = sh.sum[Geo<CLB>::at(0, lc)];
        const double rho = same ? rr : sh.sum[Geo<CLB>::at(1, lc)];
        float b32;
        if (krylov_rule_direction(S, rr, rho, K.tol2, b32)) { sh.f1[lc] = b32; sh.act[lc] = 1; }
    });
    bool act[4], any_act = false;
    float b32[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { act[j] = sh.act[4 * g.cl + j] != 0; b32[j] = sh.f1[4 * g.cl + j]; any_act |= act[j]; }
    if (!g.in || !any_act) return;
    for (int jl = 0; jl < Geo<CLB>::CL; ++jl) {
        leaf_rows(g, K, g.leaf(jl), [&](int64_t row, int64_t off) {
            float r[4], p[4];
            ldw4(K.r, off, r);
            ldw4(K.p, off, p);
            if (K.minv) {
                const float d = K.minv[row];
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = d * r[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bp = b32[j] * p[j];
                const float pn = r[j] + bp;
                p[j] = act[j] ? pn : p[j];
            }
            stw4(K.p, off, p);
        });
    }
}

// BiCGSTAB: alpha = rho / (rhat, v); s = r - alpha v, stored over r; the partials of (s, s)
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_bicg_s_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const int slots[1] = {kSlotDen};
    sum_partials<CLB, 1>(g, K.parts, K.groups, K.ldw, slots, 1, any, sh.sum);
    scalar_phase(g, K, [&](int lc, double* S) {
        if (frozen(S)) return;
        const double den = sh.sum[Geo<CLB>::at(0, lc)];
        float a32;
        if (krylov_rule_alpha<true>(S, den, a32)) { sh.f1[lc] = a32; sh.act[lc] = 1; }
    });
    bool act[4], any_act = false;
    float a32[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { act[j] = sh.act[4 * g.cl + j] != 0; a32[j] = sh.f1[4 * g.cl + j]; any_act |= act[j]; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (g.in && any_act) {
        subtree<CLB, 4>(g, [&](int t, double* cur) {
            leaf_rows(g, K, t, [&](int64_t, int64_t off) {
                float r[4], v[4];
                ldw4(K.r, off, r);
                ldw4(K.q, off, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float av = a32[j] * v[j];
                    const float rn = r[j] - av;
                    r[j] = act[j] ? rn : r[j];
                }
                stw4(K.r, off, r);
                add_dot(cur, r, r);
            });
        }, acc);
    }
    block_reduce<CLB, 1>(g, acc, sh.sum);
    if (any_act) write_partial(g, K.parts, K.groups, K.ldw, kSlotSs, acc);
}

// BiCGSTAB: (s, s) within the tolerance: x += alpha p and done.  Otherwise omega = (t, s) / (t, t); x += alpha p; x += omega s;
// r = s - omega t; the partials of (r, r) and (rhat, r)
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_bicg_x_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const int slots[3] = {kSlotSs, kSlotTs, kSlotTt};
    sum_partials<CLB, 3>(g, K.parts, K.groups, K.ldw, slots, 3, any, sh.sum);
    scalar_phase(g, K, [&](int lc, double* S) {
        sh.f1[lc] = (float)S[kKsAlpha];
        if (frozen(S)) return;
        const double ss = sh.sum[Geo<CLB>::at(0, lc)], ts = sh.sum[Geo<CLB>::at(1, lc)], tt = sh.sum[Geo<CLB>::at(2, lc)];
        float w32;
        const int act = krylov_rule_bicg_omega(S, ss, ts, tt, K.tol2, w32);
        if (act) sh.act[lc] = act;
        if (act == 2) sh.f2[lc] = w32;
    });
    int act[4];          // 1 the half step, 2 the whole
    bool any_act = false, any_whole = false;
    float a32[4], w32[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        act[j] = sh.act[4 * g.cl + j]; a32[j] = sh.f1[4 * g.cl + j]; w32[j] = sh.f2[4 * g.cl + j];
        any_act |= act[j] != 0; any_whole |= act[j] == 2;
    }
    const int nc = cols_of(g, K.m), wx = width_of(K.x, K.ld_x);
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
    if (g.in && any_act) {
        subtree<CLB, 8>(g, [&](int t, double* cur) {
            leaf_rows(g, K, t, [&](int64_t row, int64_t off) {
                float x[4], p[4];
                const int64_t offx = row * K.ld_x + g.col;
                ldv(K.x, offx, wx, nc, x);
                ldw4(K.p, off, p);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ap = a32[j] * p[j];
                    const float xn = x[j] + ap;
                    x[j] = act[j] ? xn : x[j];
                }
                if (any_whole) {
                    float s[4], tv[4], h[4];
                    ldw4(K.r, off, s);
                    ldw4(K.t, off, tv);
                    ldw4(K.rhat, off, h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float ws = w32[j] * s[j];
                        const float xn = x[j] + ws;
                        const float wt = w32[j] * tv[j];
                        const float sn = s[j] - wt;
                        x[j] = act[j] == 2 ? xn : x[j];
                        s[j] = act[j] == 2 ? sn : s[j];
                    }
                    stw4(K.r, off, s);
                    add_dot(cur, s, s);
                    add_dot(cur + 4, h, s);
                }
                stv(K.x, offx, wx, nc, x);
            });
        }, acc);
    }
    block_reduce<CLB, 2>(g, acc, sh.sum);
    if (!any_whole) return;
    write_partial(g, K.parts, K.groups, K.ldw, kSlotRr, acc);
    write_partial(g, K.parts, K.groups, K.ldw, kSlotRho, acc + 4);
}

// BiCGSTAB: the stopping rule on the new rr, then beta = (rho' / rho) (alpha / omega); p = r + beta (p - omega v)
template <int CLB>
__global__ __launch_bounds__(kKrylovThreads) void km_bicg_p_kernel(KrylovMultiStep K) {
    __shared__ Shared sh;
    const Geo<CLB> g(K.ldw);
    bool lm[4];
    const bool any = load_frozen(g, K, sh, lm);
    if (!__syncthreads_or(any)) { pass_on(g, K); return; }
    const int slots[2] = {kSlotRr, kSlotRho};
    sum_partials<CLB, 2>(g, K.parts, K.groups, K.ldw, slots, 2, any, sh.sum);
    scalar_phase(g, K, [&](int lc, double* S) {
        sh.f2[lc] = (float)S[kKsOmega];
        if (frozen(S)) return;
        const double rr = sh.sum[Geo<CLB>::at(0, lc)], rho = sh.sum[Geo<CLB>::at(1, lc)];
        if (krylov_rule_bicg_beta(S, rr, rho, K.tol2, sh.f1[lc])) sh.act[lc] = 1;
    });
    bool act[4], any_act = false;
    float b32[4], w32[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { act[j] = sh.act[4 * g.cl + j] != 0; b32[j] = sh.f1[4 * g.cl + j]; w32[j] = sh.f2[4 * g.cl + j]; any_act |= act[j]; }
    if (!g.in || !any_act) return;
    for (int jl = 0; jl < Geo<CLB>::CL; ++jl) {
        leaf_rows(g, K, g.leaf(jl), [&](int64_t, int64_t off) {
            float r[4], p[4], v[4];
            ldw4(K.r, off, r);
            ldw4(K.p, off, p);
            ldw4(K.q, off, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float wv = w32[j] * v[j];
                const float d = p[j] - wv;
                const float bd = b32[j] * d;
                const float pn = r[j] + bd;
                p[j] = act[j] ? pn : p[j];
            }
            stw4(K.p, off, p);
        });
    }
}

// Column lanes of a launch over m columns in `groups` chunks.  Any choice gives the same bits.  The widest tile that covers
// min(m, 64) columns keeps a row's accesses longest; but a workgroup streams 1024 rows of its whole tile, so while the grid is short of
// kFillGroups workgroups the tile narrows, down to 16 columns (64 contiguous bytes per row), and the other lanes go to the rows.
// HISPMV_KRYLOV_MULTI_TILE=<columns> (4 ... 64) takes the tile from the environment instead, for measurements and tests.
constexpr int64_t kFillGroups = 512;
int clb_of(int64_t groups, int64_t m) {
    const auto cover = [](int64_t w) { int b = 0; while ((4 << b) < w) ++b; return b; };
    int b = cover(m < kKrylovMultiTile ? m : kKrylovMultiTile);
    if (const char* e = std::getenv("HISPMV_KRYLOV_MULTI_TILE")) {
        const int forced = cover(std::atoi(e) < kKrylovMultiTile ? std::atoi(e) : kKrylovMultiTile);
        return forced < b ? forced : b;
    }
    const int floor_b = cover(m < 16 ? m : 16);
    while (b > floor_b && groups * ((m + (4 << b) - 1) / (4 << b)) < kFillGroups) --b;
    return b;
}
dim3 grid_of(int64_t groups, int64_t m, int clb) { return dim3((unsigned)(groups > 0 ? groups : 1), (unsigned)((m + (4 << clb) - 1) / (4 << clb))); }

}  // namespace

#define KM_DISPATCH(kernel, grid, s, m_, ...)                                                                                     \
    switch (clb_of(grid, m_)) {                                                                                                         \
        case 0: hipLaunchKernelGGL(kernel<0>, grid_of(grid, m_, 0), dim3(kKrylovThreads), 0, s, __VA_ARGS__); break;                 \
        case 1: hipLaunchKernelGGL(kernel<1>, grid_of(grid, m_, 1), dim3(kKrylovThreads), 0, s, __VA_ARGS__); break;                 \
        case 2: hipLaunchKernelGGL(kernel<2>, grid_of(grid, m_, 2), dim3(kKrylovThreads), 0, s, __VA_ARGS__); break;                 \
        case 3: hipLaunchKernelGGL(kernel<3>, grid_of(grid, m_, 3), dim3(kKrylovThreads), 0, s, __VA_ARGS__); break;                 \
        default: hipLaunchKernelGGL(kernel<4>, grid_of(grid, m_, 4), dim3(kKrylovThreads), 0, s, __VA_ARGS__); break;                \
    }                                                                                                                             \
    return hipGetLastError();

hipError_t launch_krylov_multi_dot(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t n, int m, int64_t ldw, double* part, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t groups = (n + kKrylovChunk - 1) / kKrylovChunk;
    KM_DISPATCH(km_dot_kernel, groups, s, m, a, ld_a, b, ld_b, n, m, ldw, part)
}
hipError_t launch_krylov_multi_dot_finish(const double* part, int64_t groups, int m, int64_t ldw, double* out, hipStream_t s) {
    KM_DISPATCH(km_dot_finish_kernel, 1, s, m, part, groups, m, ldw, out)
}
hipError_t launch_krylov_multi_init(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_init_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_step_dot(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_step_dot_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_cg_update(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_cg_update_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_direction(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_direction_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_bicg_s(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_bicg_s_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_bicg_x(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_bicg_x_kernel, k.groups, s, k.m, k) }
hipError_t launch_krylov_multi_bicg_p(const KrylovMultiStep& k, hipStream_t s) { KM_DISPATCH(km_bicg_p_kernel, k.groups, s, k.m, k) }

}  // namespace hispmv
