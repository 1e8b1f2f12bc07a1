// hispmv_gmres.h -- launchers of the restarted GMRES(m) vector kernels (hispmv_gmres.hip) and the workspace rule both the host-only
// hispmv_prep_gmres and the device entries follow.  The arithmetic, the order of every sum and the meaning of every word of the
// workspace are written down in include/hispmv.h ("Restarted GMRES"); the dot products are hispmv_krylov.h's, on its grid.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_krylov.h"

namespace hispmv {

constexpr int kGmresMaxRestart = 64;                       // HISPMV_GMRES_MAX_RESTART
constexpr int kGmresMaxBasis = kGmresMaxRestart + 1;       // basis vectors of a cycle, and the most dot products of one multi-dot pass
constexpr int kGmresDotTile = 8;                           // basis vectors one pass of the multi-dot kernel accumulates per thread
constexpr int kGmresLaunchesInner = 4;                     // multi-dot, subtract-and-dot twice, rotate-and-normalise
constexpr int kGmresLaunchesCycle = 3;                     // (r, r), the kernel that opens the cycle, the close

// GMRES's words of the scalar block, in slots no other solver of the layer reads through hispmv_krylov_status
enum GmresScalar {
    kGsJ = 13,           // the inner index of the last step that acted
    kGsCols = 14,        // completed columns of the open cycle: what the close still has to apply
};

// The workspace: the two scalar blocks and the scratch double of hispmv_krylov_abi.cpp's layout, the Givens data, the partial arrays
// (each of `gp` doubles per sum, gp = groups rounded up to 2), the basis, and with a preconditioner one vector z.
struct GmresLayout {
    int64_t groups = 0, gp = 0, stride = 0;
    int64_t off_c = 0, off_s = 0, off_gfin = 0, off_gres = 0, off_h1 = 0, off_h = 0, off_r = 0;          // bytes
    int64_t off_b2 = 0, off_rr = 0, off_ww = 0, off_pa = 0, off_pb = 0, off_v = 0, off_z = 0, work_bytes = 0;
};
constexpr int64_t kGmresStateBytes = kKrylovState * 8;
constexpr int64_t kGmresScratchOff = 2 * kGmresStateBytes;
inline GmresLayout gmres_layout(int64_t n, int64_t restart, bool with_minv) {
    GmresLayout l;
    l.groups = krylov_groups(n);
    l.gp = (l.groups > 0 ? l.groups + 1 : 2) / 2 * 2;
    l.stride = (n + 3) / 4 * 4;
    const int64_t arr = (kGmresMaxBasis + 1) * 8;          // 66 doubles: a multiple of 16 bytes
    l.off_c = 512;
    l.off_s = l.off_c + arr;
    l.off_gfin = l.off_s + arr;
    l.off_gres = l.off_gfin + arr;
    l.off_h1 = l.off_gres + arr;
    l.off_h = l.off_h1 + arr;
    l.off_r = l.off_h + arr;
    l.off_b2 = l.off_r + (int64_t)kGmresMaxRestart * kGmresMaxRestart * 8;
    l.off_rr = l.off_b2 + l.gp * 8;
    l.off_ww = l.off_rr + l.gp * 8;
    l.off_pa = l.off_ww + l.gp * 8;
    l.off_pb = l.off_pa + kGmresMaxBasis * l.gp * 8;
    l.off_v = l.off_pb + kGmresMaxBasis * l.gp * 8;
    l.off_z = l.off_v + (restart + 1) * l.stride * 4;
    l.work_bytes = l.off_z + (with_minv ? l.stride * 4 : 0);
    return l;
}

// The operands of one GMRES vector kernel.  As in KrylovStep, a kernel reads the scalar block s_in and its workgroup 0 writes the whole
// of s_out; only workgroup 0 writes c, s, g_fin, g_res, h1, h and R, and no kernel reads a word of these it writes itself.
struct GmresStep {
    int64_t n = 0;
    const double* s_in = nullptr;
    double* s_out = nullptr;
    double tol2 = 0, products = 0;
    int first = 0;                    // open: the first cycle, the block from nothing
    int j = 0;                        // the inner index: w is basis vector j + 1, the pass runs over basis vectors 0 .. j
    int second = 0;                   // subtract-and-dot: pass 2
    int64_t gp = 0;                   // doubles between the partial arrays of two sums
    float* V = nullptr;               // the basis, `stride` floats apart
    int64_t stride = 0;
    float* x = nullptr;
    const float* minv = nullptr;      // the inverse diagonal; the block-Jacobi variant (bs > 0 below): the block area of the buffer
    float* z = nullptr;               // minv * v_j, the operand of the next product (with minv only)
    const double* parts_in = nullptr; // subtract-and-dot: the partials it sums
    double* parts_out = nullptr;      // pass 1: the partials of pass 2
    double *part_b2 = nullptr, *part_rr = nullptr, *part_ww = nullptr;
    double *c = nullptr, *s = nullptr, *g_fin = nullptr, *g_res = nullptr, *h1 = nullptr, *h = nullptr, *R = nullptr;
};

// part[i * gp + g] = the partial of workgroup g of (V + i * ld, w), i < k <= kGmresMaxBasis; s_in given: a frozen solve writes nothing
hipError_t launch_gmres_multi_dot(const float* V, int64_t ld, int64_t k, const float* w, int64_t n, double* part, int64_t gp, const double* s_in,
                                  hipStream_t s);
// out[i] = the sum of part[i * gp .. + groups) in the fixed order, i < k (one workgroup)
hipError_t launch_gmres_dot_finish(const double* part, int64_t gp, int64_t groups, int64_t k, double* out, hipStream_t s);
// The three kernels that precondition take bs: 0 = k.minv is an inverse diagonal, 4 / 8 / 16 / 32 = the block area of a block-Jacobi
// buffer of that block size (hispmv_block_jacobi_device.h); everything else is the same text.
hipError_t launch_gmres_open(const GmresStep& k, hipStream_t s, int bs = 0);          // the stopping rule on (r, r); v_0 = r / beta
hipError_t launch_gmres_sub(const GmresStep& k, hipStream_t s);                       // w -= sum h_i v_i; the partials of the next pass
hipError_t launch_gmres_rotate(const GmresStep& k, hipStream_t s, int bs = 0);        // the Givens step and the stopping rule; v_{j+1} = w / hn
hipError_t launch_gmres_close(const GmresStep& k, hipStream_t s, int bs = 0);         // R y = g; x += minv * V y

}  // namespace hispmv
