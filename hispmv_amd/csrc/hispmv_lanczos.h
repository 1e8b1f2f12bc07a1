// hispmv_lanczos.h -- launchers of the kernels the two thick-restart solvers add (hispmv_lanczos.hip) and the workspace rule the
// host-only hispmv_prep_lanczos and hispmv_prep_gk and the device entries follow.  The arithmetic and the meaning of every word of the
// workspace are written down in include/hispmv.h ("Lanczos / eigsh", "Golub-Kahan / svds").  A Lanczos step with full
// reorthogonalisation is a GMRES inner iteration without the Givens rotation, and a Golub-Kahan step is two Lanczos steps on two bases
// of different lengths: the multi-dot and the subtract-and-dot kernels are hispmv_gmres.h's, launched as they are; this file adds the
// kernel that opens a run, the kernel that normalises and records a step -- one text under three rules -- and the basis rotation of a
// restart.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

#include "hispmv_gmres.h"

namespace hispmv {

constexpr int kLanczosMaxNcv = kGmresMaxRestart;           // HISPMV_LANCZOS_MAX_NCV, HISPMV_GK_MAX_NCV: V holds ncv + 1 <= kGmresMaxBasis vectors, U ncv
constexpr int kLanczosLaunchesStep = 5;                    // the product, multi-dot, subtract-and-dot twice, normalise-and-record
constexpr int kLanczosHcLd = kGmresMaxBasis + 1;           // doubles between two columns of Hc (Golub-Kahan: Gc)
constexpr double kLanczosTiny2 = 1.0 / (4096.0 * 4096.0);  // tiny^2, tiny = 2^-12: the invariant subspace rule
constexpr int kRotateMaxIn = kGmresMaxBasis;               // basis_rotate: m <= 65 inputs ...
constexpr int kRotateMaxOut = kGmresMaxRestart;            // ... k <= 64 outputs
constexpr int kRotateElems = 2;                            // elements of a thread (the register budget)
constexpr int kRotateThreads = 256;
constexpr int kRotateGroup = 16;                           // coefficients of one uniform load
constexpr int64_t kRotateSplitBelow = 256 * 1024;          // n below which the columns are split over a workgroup's wavefronts

// The two solvers' words of the scalar block, in the slots GMRES uses for its own (no other kernel of the layer reads them)
enum LanczosScalar {
    kLsSteps = 13,          // steps done: the order m of the projected matrix
    kLsInvariant = 14,      // the last step found an invariant subspace (kKsDone is set with it: that freezes the later kernels)
    kLsClosedU = 15,        // Golub-Kahan: the U side closed the space: A V_steps lies in span U (set with invariant and kKsDone)
};

// The workspace: three scalar blocks (a step's kernels pass the state on by one rule, which for Lanczos's three
// kernels gives 0 -> 1 -> 2 -> 0) in the 512 bytes the other solvers open with, h1 and h (66 doubles each; Golub-Kahan's g1 and g,
// used by the two sides in turn), `arrays` columns of 66 doubles (Hc: 64; Gc: 64 and the alphas as a 65th), the betas (66 doubles),
// Yt (64 x 65 floats; Golub-Kahan's two rotations of a look use it in turn), the partial arrays (gp doubles per sum, as in
// gmres_layout; Golub-Kahan: gp from the larger of the two grids) and the basis V; Golub-Kahan's U lies behind it.
struct LanczosLayout {
    int64_t groups = 0, gp = 0, stride = 0;
    int64_t off_h1 = 0, off_h = 0, off_hc = 0, off_beta = 0, off_yt = 0;          // bytes
    int64_t off_vv = 0, off_ww = 0, off_pa = 0, off_pb = 0, off_v = 0, work_bytes = 0;
    int64_t off_alpha = 0, off_u = 0, stride_u = 0;                               // Golub-Kahan only
};
inline LanczosLayout basis_layout(int64_t groups, int64_t n, int64_t ncv, int64_t arrays) {
    LanczosLayout l;
    l.groups = groups;
    l.gp = (l.groups > 0 ? l.groups + 1 : 2) / 2 * 2;
    l.stride = (n + 3) / 4 * 4;
    const int64_t arr = (int64_t)kLanczosHcLd * 8;
    l.off_h1 = 512;
    l.off_h = l.off_h1 + arr;
    l.off_hc = l.off_h + arr;
    l.off_beta = l.off_hc + arrays * arr;
    l.off_yt = l.off_beta + arr;
    l.off_vv = l.off_yt + (int64_t)kRotateMaxOut * kRotateMaxIn * 4;
    l.off_ww = l.off_vv + l.gp * 8;
    l.off_pa = l.off_ww + l.gp * 8;
    l.off_pb = l.off_pa + kGmresMaxBasis * l.gp * 8;
    l.off_v = l.off_pb + kGmresMaxBasis * l.gp * 8;
    l.work_bytes = l.off_v + (ncv + 1) * l.stride * 4;
    return l;
}
inline LanczosLayout lanczos_layout(int64_t n, int64_t ncv) { return basis_layout(krylov_groups(n), n, ncv, kLanczosMaxNcv); }
inline LanczosLayout gk_layout(int64_t rows, int64_t cols, int64_t ncv) {
    LanczosLayout l = basis_layout(std::max(krylov_groups(rows), krylov_groups(cols)), cols, ncv, kLanczosMaxNcv + 1);
    l.off_alpha = l.off_hc + (int64_t)kLanczosMaxNcv * kLanczosHcLd * 8;
    l.stride_u = (rows + 3) / 4 * 4;
    l.off_u = l.work_bytes;
    l.work_bytes = l.off_u + ncv * l.stride_u * 4;
    return l;
}

// The operands of the open and the record kernel on the Krylov grid of n.  As in GmresStep: a kernel reads s_in, its workgroup 0 writes
// the whole of s_out, only workgroup 0 writes Hc, alpha and beta, and no kernel reads a word of these it writes.
struct RecordStep {
    int64_t n = 0;                     // Golub-Kahan: rows on the U side, cols on the V side
    const double* s_in = nullptr;
    double* s_out = nullptr;
    int j = 0;                         // record: the step; w is basis vector j + 1 (Golub-Kahan's U side: j)
    const float* v0 = nullptr;         // open: the start vector
    float* V = nullptr;                // the basis w lies in
    int64_t stride = 0;
    const double* part = nullptr;      // open: the partials of (v0, v0); record: of (w, w)
    const double* h = nullptr;         // record: the coefficients of this step, j + 1 of them (Golub-Kahan's U side: j)
    double* Hc = nullptr;              // Lanczos, Golub-Kahan's U side: column j
    double* beta = nullptr;            // Lanczos, Golub-Kahan's V side
    double* alpha = nullptr;           // Golub-Kahan's U side
};

// The three rules of the record kernel.  All: ww = (w, w), the closing rule ww <= tiny^2 * (ww + sum h_i^2), w / sqrt(ww) in place.
enum RecordRule {
    kRecordLanczos = 0,          // Hc column j, beta_j, steps = j + 1, one more product; the rule: invariant
    kRecordGkU = 1,              // Gc column j, alpha_j; the rule closes the space: steps = j, one more product, invariant and closed_u
    kRecordGkV = 2,              // beta_j, steps = j + 1, two more products; the rule: invariant
};

hipError_t launch_lanczos_open(const RecordStep& k, hipStream_t s);                      // the block from nothing; V_0 = v0 / |v0|
hipError_t launch_basis_record(const RecordStep& k, RecordRule rule, hipStream_t s);     // the end of a (side of a) step under `rule`
// out[c * ld_out + e] = sum_{i < m} Yt[c * m + i] * V[i * ld_v + e] for c < k, e < n, i ascending from 0.0f, fp32 and unfused;
// 1 <= m <= kRotateMaxIn, 1 <= k <= kRotateMaxOut.  out may be V with ld_out = ld_v.  xdst given: xdst[e] = xsrc[e] as well, xsrc read
// with the inputs (xdst may be one of them).
hipError_t launch_basis_rotate(const float* V, int64_t ld_v, int m, int k, const float* Yt, float* out, int64_t ld_out, int64_t n, const float* xsrc,
                               float* xdst, hipStream_t s);

}  // namespace hispmv
