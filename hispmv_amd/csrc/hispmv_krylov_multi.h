// hispmv_krylov_multi.h -- launchers of the multi-right-hand-side Krylov kernels (hispmv_krylov_multi.hip): the vector kernels of
// hispmv_krylov.h over num_vecs independent columns of feature-major operands [n, ld], lanes across columns.  Column v computes what
// the single-vector kernels compute for a vector of n elements, bit for bit: the same scalar block (KrylovScalar), the same partial
// arrays (KrylovSlot), the same order of every sum (include/hispmv.h).  The workspace is hispmv_krylov_multi_abi.cpp's, the loop hispmv_krylov_solve.h's.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_krylov.h"

namespace hispmv {

constexpr int64_t kKrylovMultiMaxN = (int64_t)kKrylovChunk * kKrylovMaxGroups;   // every workgroup owns exactly one chunk
constexpr int64_t kKrylovMultiMaxVecs = 1 << 20;
constexpr int kKrylovMultiTile = 64;                                             // columns of the widest column tile (16 lanes x 4)

// The rule of hispmv_prep_krylov_multi.  The workspace of a solve: two arrays of scalar blocks [ldw][kKrylovState] (a kernel reads one
// and writes the other) and one row of ldw doubles for the (b_v, b_v) the host looks at; the partials [kKrylovSlots][groups][ldw];
// the solver's vectors, each [n, ldw] floats; the workspace of hispmv_spmm_device.
struct KrylovMultiLayout {
    int64_t groups = 0;          // ceil(n / 1024): workgroups per column tile, partials per column
    int64_t ldw = 0;             // leading dimension of the workspace's vectors, partials and scalar blocks: num_vecs rounded up to 4
    int64_t state_bytes = 0;     // byte offset of the partials
    int64_t part_bytes = 0;      // state_bytes + part_bytes = byte offset of the first vector (R)
};
inline KrylovMultiLayout krylov_multi_layout(int64_t n, int64_t num_vecs) {
    KrylovMultiLayout l;
    l.groups = (n + kKrylovChunk - 1) / kKrylovChunk;
    l.ldw = (num_vecs + 3) / 4 * 4;
    l.state_bytes = 2 * l.ldw * kKrylovState * 8 + l.ldw * 8;
    l.part_bytes = (int64_t)kKrylovSlots * l.groups * l.ldw * 8;
    return l;
}

// The operands of one kernel.  Scalar blocks: s_in / s_out + column * kKrylovState.  Partials: parts + (slot * groups + g) * ldw +
// column.  x is the caller's [n, ld_x] (columns at or beyond m never touched); every other vector is the workspace's [n, ldw].
struct KrylovMultiStep {
    int64_t n = 0;
    int m = 0;                      // num_vecs
    int64_t ldw = 0, groups = 0;
    const double* s_in = nullptr;
    double* s_out = nullptr;
    double* parts = nullptr;
    double tol2 = 0, products = 0;
    int first = 0;
    int slot_rho = kSlotRho;
    float* x = nullptr;
    int64_t ld_x = 0;
    const float* minv = nullptr;    // [n], shared by all columns
    float* r = nullptr;
    float* p = nullptr;
    const float* q = nullptr;
    float* rhat = nullptr;
    const float* t = nullptr;
    const float *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr;
    int slot1 = 0, slot2 = 0;
};

// part[g * ldw + v] = the partial of chunk g of (a[:, v], b[:, v]), v < m; a is [n, ld_a], b is [n, ld_b], columns at or beyond m not read
hipError_t launch_krylov_multi_dot(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t n, int m, int64_t ldw, double* part, hipStream_t s);
// out[v] = the sum of column v's partials in the fixed order, v < m
hipError_t launch_krylov_multi_dot_finish(const double* part, int64_t groups, int m, int64_t ldw, double* out, hipStream_t s);
hipError_t launch_krylov_multi_init(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_step_dot(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_cg_update(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_direction(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_bicg_s(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_bicg_x(const KrylovMultiStep& k, hipStream_t s);
hipError_t launch_krylov_multi_bicg_p(const KrylovMultiStep& k, hipStream_t s);

}  // namespace hispmv
