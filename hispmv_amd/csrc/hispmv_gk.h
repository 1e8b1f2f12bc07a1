// hispmv_gk.h -- the launcher of the one kernel thick-restart Golub-Kahan bidiagonalisation adds (hispmv_gk.hip) and the workspace rule
// the host-only hispmv_prep_gk and the device entries follow.  The arithmetic and the meaning of every word of the workspace are written
// down in include/hispmv.h ("Golub-Kahan / svds").  A step is two Lanczos steps on two bases of different lengths: the product, the
// multi-dot and the subtract-and-dot kernels are launched as they are (hispmv_gmres.h), the open is Lanczos's on V slot 0, the restart
// and the finish are basis_rotate (hispmv_lanczos.h); this file adds the kernel that normalises and records, for either side.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

#include "hispmv_lanczos.h"

namespace hispmv {

constexpr int kGkMaxNcv = kLanczosMaxNcv;          // HISPMV_GK_MAX_NCV: V holds ncv + 1 <= kGmresMaxBasis vectors, U ncv
constexpr int kGkLaunchesStep = 10;                // two products; per side a multi-dot, subtract-and-dot twice, normalise-and-record
constexpr int kGkGcLd = kLanczosHcLd;              // doubles between two columns of Gc

// Golub-Kahan's words of the scalar block: steps and invariant where Lanczos keeps them, closed_u in the slot no solver uses
enum GkScalar {
    kGkSteps = kLsSteps,
    kGkInvariant = kLsInvariant,
    kGkClosedU = 15,        // the U side closed the space: A V_steps lies in span U (set with invariant and kKsDone)
};

// The workspace: three scalar blocks in the 512 bytes the other solvers open with, g1 and g (66 doubles each, used by the two sides in
// turn), Gc (64 columns of 66 doubles), the alphas and the betas (66 doubles each, right behind Gc), Yt (64 x 65 floats, used by the
// two rotations of a look in turn), the partial arrays (gp doubles per sum, gp from the larger of the two grids), V, then U.
struct GkLayout {
    int64_t groups = 0, gp = 0, stride_v = 0, stride_u = 0;
    int64_t off_g1 = 0, off_g = 0, off_gc = 0, off_alpha = 0, off_beta = 0, off_yt = 0;          // bytes
    int64_t off_vv = 0, off_ww = 0, off_pa = 0, off_pb = 0, off_v = 0, off_u = 0, work_bytes = 0;
};
inline GkLayout gk_layout(int64_t rows, int64_t cols, int64_t ncv) {
    GkLayout l;
    l.groups = std::max(krylov_groups(rows), krylov_groups(cols));
    l.gp = (l.groups > 0 ? l.groups + 1 : 2) / 2 * 2;
    l.stride_v = (cols + 3) / 4 * 4;
    l.stride_u = (rows + 3) / 4 * 4;
    const int64_t arr = (int64_t)kGkGcLd * 8;
    l.off_g1 = 512;
    l.off_g = l.off_g1 + arr;
    l.off_gc = l.off_g + arr;
    l.off_alpha = l.off_gc + kGkMaxNcv * arr;
    l.off_beta = l.off_alpha + arr;
    l.off_yt = l.off_beta + arr;
    l.off_vv = l.off_yt + (int64_t)kRotateMaxOut * kRotateMaxIn * 4;
    l.off_ww = l.off_vv + l.gp * 8;
    l.off_pa = l.off_ww + l.gp * 8;
    l.off_pb = l.off_pa + kGmresMaxBasis * l.gp * 8;
    l.off_v = l.off_pb + kGmresMaxBasis * l.gp * 8;
    l.off_u = l.off_v + (ncv + 1) * l.stride_v * 4;
    l.work_bytes = l.off_u + ncv * l.stride_u * 4;
    return l;
}

// The operands of the normalise-and-record kernel on the Krylov grid of its side's n.  As in LanczosStep: the kernel reads s_in, its
// workgroup 0 writes the whole of s_out, only workgroup 0 writes Gc, alpha and beta, and it reads no word of these it writes.
struct GkStep {
    int64_t n = 0;                     // rows on the U side, cols on the V side
    const double* s_in = nullptr;
    double* s_out = nullptr;
    int j = 0;                         // the step: the U side works on U slot j, the V side on V slot j + 1
    float* W = nullptr;                // the side's basis
    int64_t stride = 0;
    const double* part = nullptr;      // the partials of (w, w)
    const double* g = nullptr;         // the side's coefficients of this step: j of them on the U side, j + 1 on the V side
    double* Gc = nullptr;              // U side: column j
    double* alpha = nullptr;           // U side
    double* beta = nullptr;            // V side
};

// side 0: Gc column j, alpha_j, the closed-space rule; U_j = u / alpha_j.  side 1: beta_j, the invariant rule; V_{j+1} = w / beta_j
hipError_t launch_gk_record(const GkStep& k, int side, hipStream_t s);

}  // namespace hispmv
