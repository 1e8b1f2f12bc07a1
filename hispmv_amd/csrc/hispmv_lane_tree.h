// hispmv_lane_tree.h -- the sum over the 64 lanes of a wavefront, 64 elements at a time, of the wide-batch value-gradient kernels
// (hispmv_spmm_grad.hip, fp32 and bf16 operands alike).  Device code only; include it behind hispmv_slice_walk.h (f2i, i2f).
#pragma once
#include <hip/hip_runtime.h>

#include "hispmv_slice_walk.h"

namespace hispmv {

namespace {

// ---- the sum over the 64 lanes, 64 elements at a time -----------------------------------------------------------------------------
// a, b: the per-lane partials of two elements (level 0), or two values that each hold, in every lane, the sum over the lane's block of
// 2^LV lanes of one of 2^LV elements -- the element the lane's low LV bits name.  The merge keeps a in the lanes whose bit LV is 0 and b
// in the others and adds the partner lane's (lane ^ 2^LV) copy of the same value: the result holds sums over blocks of 2^(LV + 1) lanes
// of 2^(LV + 1) elements, a's where bit LV of the lane is 0.  Level 0 adds lanes (2i, 2i + 1), level 1 pairs of pairs, and so on: the
// tree of every element is the same pairwise tree, whichever lanes it ends in (IEEE addition commutes).
//   xor 1, 2: select, select, DPP quad_perm, add.     xor 8: the same with DPP row_ror:8.
//   xor 4: no row operation swaps the banks of a row, so the partner's copy arrives by row_shl:4 for a (read in the lanes with bit 2
//          clear) and by row_shr:4 for b (read in the others): add, add, select.
//   xor 16, 32: v_permlane16_swap / v_permlane32_swap (gfx950) exchange the odd rows (upper half) of a with the even rows (lower half)
//          of b; after it the two registers ARE kept and partner's copy, so the merge is swap, add -- no select.
template <int CTRL> __device__ __forceinline__ float dpp_move(float v) {
    return i2f(__builtin_amdgcn_update_dpp(0, f2i(v), CTRL, 0xf, 0xf, true));
}
template <int LV> __device__ __forceinline__ float merge(float a, float b, int lane) {
    if constexpr (LV == 0 || LV == 1 || LV == 3) {
        constexpr int ctrl = LV == 0 ? 0xB1 /* quad_perm:[1,0,3,2] */ : LV == 1 ? 0x4E /* quad_perm:[2,3,0,1] */ : 0x128 /* row_ror:8 */;
        const bool hi = (lane >> LV) & 1;
        const float keep = hi ? b : a, send = hi ? a : b;
        return keep + dpp_move<ctrl>(send);
    } else if constexpr (LV == 2) {
        const float sa = a + dpp_move<0x104 /* row_shl:4: lane l reads lane l + 4 */>(a);
        const float sb = b + dpp_move<0x114 /* row_shr:4: lane l reads lane l - 4 */>(b);
        return (lane & 4) ? sb : sa;
    } else if constexpr (LV == 4) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)f2i(a), (unsigned)f2i(b), false, false);
        return i2f((int)r[0]) + i2f((int)r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)f2i(a), (unsigned)f2i(b), false, false);
        return i2f((int)r[0]) + i2f((int)r[1]);
    }
}
// The "binary counter" of one element position k: slot[LV - 1] holds a value of level LV that waits for its partner.  Pair P (0 .. 31)
// of a step brings the level-1 value of lanes 2P and 2P + 1's elements; it is merged upwards as far as the bits of P carry.  Behind pair
// 31 the return value is the level-6 value: lane L holds the total of the element of lane L.  (P is wave-uniform: scalar branches.)
struct Counter { float slot[5]; };
__device__ __forceinline__ float counter_push(Counter& c, float t, int P, int lane) {
    if (!(P & 1)) { c.slot[0] = t; return t; }
    t = merge<1>(c.slot[0], t, lane);
    if (!(P & 2)) { c.slot[1] = t; return t; }
    t = merge<2>(c.slot[1], t, lane);
    if (!(P & 4)) { c.slot[2] = t; return t; }
    t = merge<3>(c.slot[2], t, lane);
    if (!(P & 8)) { c.slot[3] = t; return t; }
    t = merge<4>(c.slot[3], t, lane);
    if (!(P & 16)) { c.slot[4] = t; return t; }
    return merge<5>(c.slot[4], t, lane);
}

}  // namespace

}  // namespace hispmv
