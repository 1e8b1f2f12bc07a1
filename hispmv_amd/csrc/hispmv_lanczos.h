// hispmv_lanczos.h -- launchers of the thick-restart Lanczos kernels (hispmv_lanczos.hip) and the workspace rule the host-only
// hispmv_prep_lanczos and the device entries follow.  The arithmetic and the meaning of every word of the workspace are written down
// in include/hispmv.h ("Lanczos / eigsh").  A Lanczos step with full reorthogonalisation is a GMRES inner iteration without the Givens
// rotation: the multi-dot and the subtract-and-dot kernels are hispmv_gmres.h's, launched as they are; this file adds the kernel that
// opens a run, the kernel that normalises and records a step, and the basis rotation of a restart.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "hispmv_gmres.h"

namespace hispmv {

constexpr int kLanczosMaxNcv = kGmresMaxRestart;           // HISPMV_LANCZOS_MAX_NCV: the basis holds ncv + 1 <= kGmresMaxBasis vectors
constexpr int kLanczosLaunchesStep = 5;                    // the product, multi-dot, subtract-and-dot twice, normalise-and-record
constexpr int kLanczosHcLd = kGmresMaxBasis + 1;           // doubles between two columns of Hc
constexpr double kLanczosTiny2 = 1.0 / (4096.0 * 4096.0);  // tiny^2, tiny = 2^-12: the invariant subspace rule
constexpr int kRotateMaxIn = kGmresMaxBasis;               // basis_rotate: m <= 65 inputs ...
constexpr int kRotateMaxOut = kGmresMaxRestart;            // ... k <= 64 outputs
constexpr int kRotateElems = 2;                            // elements of a thread (the register budget)
constexpr int kRotateThreads = 256;
constexpr int kRotateGroup = 16;                           // coefficients of one uniform load
constexpr int64_t kRotateSplitBelow = 256 * 1024;          // n below which the columns are split over a workgroup's wavefronts

// Lanczos's words of the scalar block, in the slots GMRES uses for its own (no other kernel of the layer reads them)
enum LanczosScalar {
    kLsSteps = 13,          // steps done: the order m of the projected matrix
    kLsInvariant = 14,      // the last step found an invariant subspace (kKsDone is set with it: that freezes the later kernels)
};

// The workspace: three scalar blocks (a step's kernels pass the state 0 -> 1 -> 2 -> 0) in the 512 bytes the other solvers open
// with, h1 and h (66 doubles each), Hc (64 columns of 66
// doubles), the betas (66 doubles), Yt (64 x 65 floats), the partial arrays (gp doubles per sum, as in gmres_layout) and the basis.
struct LanczosLayout {
    int64_t groups = 0, gp = 0, stride = 0;
    int64_t off_h1 = 0, off_h = 0, off_hc = 0, off_beta = 0, off_yt = 0;          // bytes
    int64_t off_vv = 0, off_ww = 0, off_pa = 0, off_pb = 0, off_v = 0, work_bytes = 0;
};
inline LanczosLayout lanczos_layout(int64_t n, int64_t ncv) {
    LanczosLayout l;
    l.groups = krylov_groups(n);
    l.gp = (l.groups > 0 ? l.groups + 1 : 2) / 2 * 2;
    l.stride = (n + 3) / 4 * 4;
    const int64_t arr = (int64_t)kLanczosHcLd * 8;
    l.off_h1 = 512;
    l.off_h = l.off_h1 + arr;
    l.off_hc = l.off_h + arr;
    l.off_beta = l.off_hc + kLanczosMaxNcv * arr;
    l.off_yt = l.off_beta + arr;
    l.off_vv = l.off_yt + (int64_t)kRotateMaxOut * kRotateMaxIn * 4;
    l.off_ww = l.off_vv + l.gp * 8;
    l.off_pa = l.off_ww + l.gp * 8;
    l.off_pb = l.off_pa + kGmresMaxBasis * l.gp * 8;
    l.off_v = l.off_pb + kGmresMaxBasis * l.gp * 8;
    l.work_bytes = l.off_v + (ncv + 1) * l.stride * 4;
    return l;
}

// The operands of the two Lanczos kernels on the Krylov grid.  As in GmresStep: a kernel reads s_in, its workgroup 0 writes the whole
// of s_out, only workgroup 0 writes Hc and beta, and no kernel reads a word of these it writes.
struct LanczosStep {
    int64_t n = 0;
    const double* s_in = nullptr;
    double* s_out = nullptr;
    int j = 0;                         // norm: the step; w is basis vector j + 1
    const float* v0 = nullptr;         // open: the start vector
    float* V = nullptr;
    int64_t stride = 0;
    const double* part = nullptr;      // open: the partials of (v0, v0); norm: of (w, w)
    const double* h = nullptr;         // norm: h_0 .. h_j of this step
    double* Hc = nullptr;
    double* beta = nullptr;
};

hipError_t launch_lanczos_open(const LanczosStep& k, hipStream_t s);          // the block from nothing; V_0 = v0 / |v0|
hipError_t launch_lanczos_norm(const LanczosStep& k, hipStream_t s);          // Hc column j, beta_j, the invariant rule; V_{j+1} = w / beta_j
// out[c * ld_out + e] = sum_{i < m} Yt[c * m + i] * V[i * ld_v + e] for c < k, e < n, i ascending from 0.0f, fp32 and unfused;
// 1 <= m <= kRotateMaxIn, 1 <= k <= kRotateMaxOut.  out may be V with ld_out = ld_v.  xdst given: xdst[e] = xsrc[e] as well, xsrc read
// with the inputs (xdst may be one of them).
hipError_t launch_basis_rotate(const float* V, int64_t ld_v, int m, int k, const float* Yt, float* out, int64_t ld_out, int64_t n, const float* xsrc,
                               float* xdst, hipStream_t s);

}  // namespace hispmv
