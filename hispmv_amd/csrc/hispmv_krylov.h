// hispmv_krylov.h -- launchers of the Krylov layer's vector kernels (hispmv_krylov.hip): the fixed-order fp64 dot product of fp32
// vectors and the fused updates of CG, BiCGSTAB and CGLS that keep every scalar on the device.  The workspace layout is
// hispmv_krylov_abi.cpp's, the solve loop hispmv_krylov_solve.h's, the scalar rules hispmv_krylov_scalar.h's; the arithmetic and the
// order of every sum are written down in include/hispmv.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hispmv {

constexpr int kKrylovChunk = 1024;          // elements of a chunk: 256 threads x 4 consecutive floats
constexpr int kKrylovThreads = 256;
constexpr int kKrylovMaxGroups = 1024;      // workgroups of a pass = partials of a dot product
constexpr int kKrylovState = 16;            // doubles of a scalar block
constexpr int kKrylovSlots = 8;             // partial arrays of kKrylovMaxGroups doubles each

// workgroups (and fp64 partials) of a pass over n elements: the rule of hispmv_prep_krylov_groups
inline int64_t krylov_groups(int64_t n) {
    const int64_t chunks = (n + kKrylovChunk - 1) / kKrylovChunk;
    return chunks < kKrylovMaxGroups ? chunks : kKrylovMaxGroups;
}

// the scalar block (doubles) ...
enum KrylovScalar {
    kKsRho = 0,          // (r, z) of CG, (rhat, r) of BiCGSTAB, (s, s) of CGLS
    kKsDen = 1,          // the last denominator: (p, q), (rhat, v), (q, q)
    kKsRr = 2,           // what the stopping rule compares: (r, r); CGLS (s, s)
    kKsBb = 3,           // its reference: (b, b); CGLS (A^T b, A^T b)
    kKsB2 = 4,           // (b, b)
    kKsAlpha = 5,
    kKsOmega = 6,
    kKsIters = 7,        // updates of x applied
    kKsDone = 8,
    kKsBreakdown = 9,
    kKsProducts = 10,    // products the call enqueues in all (written by the first kernel; what hispmv_krylov_status reports)
    kKsTs = 11,          // BiCGSTAB: (t, s)
    kKsTt = 12,          //           (t, t)
};
// ... and the partial arrays of the workspace
enum KrylovSlot { kSlotB2 = 0, kSlotBb = 1, kSlotRr = 2, kSlotRho = 3, kSlotDen = 4, kSlotSs = 5, kSlotTs = 6, kSlotTt = 7 };

// The operands of one vector kernel.  Every kernel of a solve reads the scalar block s_in (written by the kernel before it) and its
// workgroup 0 writes the whole of s_out, the other of the two blocks: no kernel reads a word another workgroup of it writes.
struct KrylovStep {
    int64_t n = 0;                  // elements of the vectors the pass streams (and of the dot products it writes partials of)
    int64_t n2 = 0;                 // CGLS update: elements of r and q (n: of x and p)
    const double* s_in = nullptr;
    double* s_out = nullptr;
    double* parts = nullptr;        // kKrylovSlots x kKrylovMaxGroups
    double tol2 = 0;                // rtol * rtol
    double products = 0;
    int first = 0;                  // the pass behind the first product: rho and rr still lie in their partials (slot_rho, kSlotRr)
    int slot_rho = kSlotRho;        // where rho's partials lie (without minv, and in CGLS: kSlotRr, rho is rr)
    int slot_bb = kSlotB2;          // init: where (reference, reference) lies
    float* x = nullptr;
    const float* minv = nullptr;    // the inverse diagonal; the block-Jacobi variants (bs > 0 below): the block area of the buffer
    float* r = nullptr;             // CGLS direction pass: s
    float* p = nullptr;
    const float* q = nullptr;       // BiCGSTAB: v
    float* rhat = nullptr;
    const float* t = nullptr;
    // the dot pass: (a1, b1) -> slot1 and, a2 given, (a2, b2) -> slot2
    const float *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr;
    int slot1 = 0, slot2 = 0;
};

// part[g] = the partial of workgroup g of (a, b), g < krylov_groups(n)
hipError_t launch_krylov_dot(const float* a, const float* b, int64_t n, double* part, hipStream_t s);
// *out = the sum of the groups partials in the fixed order (one workgroup)
hipError_t launch_krylov_dot_finish(const double* part, int64_t groups, double* out, hipStream_t s);
// The three kernels that precondition take bs: 0 = k.minv is an inverse diagonal (z = minv * r elementwise), 4 / 8 / 16 / 32 = it is the
// block area of a block-Jacobi buffer of that block size (z = M^-1 r, hispmv_block_jacobi_device.h); everything else is the same text.
hipError_t launch_krylov_init(const KrylovStep& k, hipStream_t s, int bs = 0);           // p = z = minv * r (or r), rhat = r; partials (r, r), (r, z)
hipError_t launch_krylov_step_dot(const KrylovStep& k, hipStream_t s);       // the dot pass behind a product
hipError_t launch_krylov_cg_update(const KrylovStep& k, hipStream_t s, int bs = 0);      // x += alpha p, r -= alpha q; partials (r, r), (r, z)
hipError_t launch_krylov_direction(const KrylovStep& k, hipStream_t s, int bs = 0);      // p = z + beta p, and the stopping rule
hipError_t launch_krylov_cgls_update(const KrylovStep& k, hipStream_t s);    // x += alpha p (n), r -= alpha q (n2)
hipError_t launch_krylov_bicg_s(const KrylovStep& k, hipStream_t s);         // r = s = r - alpha v; partials (s, s)
hipError_t launch_krylov_bicg_x(const KrylovStep& k, hipStream_t s);         // x += alpha p + omega s, r = s - omega t; partials (r, r), (rhat, r)
hipError_t launch_krylov_bicg_p(const KrylovStep& k, hipStream_t s);         // p = r + beta (p - omega v), and the stopping rule

}  // namespace hispmv
