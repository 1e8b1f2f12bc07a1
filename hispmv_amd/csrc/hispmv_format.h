// hispmv_format.h -- constants of the slice-stream format shared by the host packer
// (hispmv_prep.cpp), the device packer (hispmv_plan.cpp) and the device kernels (hispmv_kernels.hip).
#pragma once
#include <cstdint>
#include <memory>
#include <utility>

namespace hispmv {

constexpr int kSliceElems = 1024;             // elements per wavefront slice
constexpr uint32_t kRowEndBit = 0x80000000u;  // host word / wide device meta: bit 31; bits 30:0 = column
constexpr uint32_t kGlobalColBit = 0x40000000u;  // wide device meta of an LDS-staged group: bits 29:0 are a column of x
                                                 // (gathered through L2), not an index into the group's window

// Device layout of one slice (structure of arrays, element order = the host stream's CSR order):
//   [values: 1024 x fp32][meta: 1024 x u16 (compact) or 1024 x u32 (wide)]
// compact meta = rowEnd<<15 | index into the workgroup's LDS window of x (< 32768): 6 bytes per element instead of the
// 8 of the reference's word (spmv-helper.h:45-60) -- every slice of a group whose elements all lie inside its window;
// wide meta = rowEnd<<31 | (kGlobalColBit | column, or window index, or plain column for groups without a window).
// A wavefront reads a slice in kSliceSteps steps of kStepElems elements, kLaneElems consecutive elements per lane and step
// (one global_load_dwordx4 of values + one dwordx2 / dwordx4 of meta per lane and step, fully coalesced).
constexpr int kLaneElems = 4;
constexpr int kStepElems = 64 * kLaneElems;               // 256
constexpr int kSliceSteps = kSliceElems / kStepElems;     // 4
constexpr uint32_t kCompactEndBit = 0x8000u;
constexpr int kCompactMaxIndex = 32768;                   // LDS window floats addressable by a compact meta
constexpr int kSliceUnit = 2048;                          // slice sizes and offsets are multiples of this many bytes
constexpr int kCompactSliceBytes = kSliceElems * 6;       // 6144 = 3 units
constexpr int kWideSliceBytes = kSliceElems * 8;          // 8192 = 4 units
// HALF slice (bf16 value storage, hispmv_set_value_storage): the compact slice with its values kept as bfloat16 -- 1024 x (bf16 value
// + the compact 16-bit meta) = 4096 B = 2 units, for every group that would be compact, stray-slot groups included.  Same element
// order, same meta encoding, same kLaneElems consecutive elements per lane and step; the 8 + 8 bytes of a lane-step are INTERLEAVED:
//   piece (step j, lane l) = 16 B at (j * 64 + l) * 16 = {v0 | v1 << 16, v2 | v3 << 16, m0 | m1 << 16, m2 | m3 << 16}
// so ONE global_load_dwordx4 per lane and step fetches everything: 4 loads in flight per slice instead of the 8 a structure of
// arrays ([1024 x bf16][1024 x u16], two dwordx2 per lane and step) needs, one address per step instead of two, and 16 VGPRs per
// slice in flight instead of the compact slice's 24 -- the slice loop is sensitive to every live register and every counted load
// (hispmv_kernels.hip: slices_group).  A wavefront still reads 1024 contiguous bytes per load.  bf16 -> fp32 is `bits << 16` (lower
// half of a dword) or `bits & 0xffff0000` (upper half): one VALU operation per element.  The structure-of-arrays variant was not built.
constexpr int kHalfSliceBytes = kSliceElems * 4;          // 4096 = 2 units
constexpr int kGroupCompact = 1, kGroupStrays = 2, kGroupHalf = 4;   // bits of groups[].w (device group table)
constexpr int kStraySlots = 64;                           // stray slots of a compact slice (hispmv_plan.h): x values one wavefront keeps behind the window
constexpr int kFixShortMax = 32;                          // a row cut over at most this many slices is finished by one thread of the tail launch, a longer chain by a wavefront

// R of the bf16 value storage: fp32 -> the nearest bfloat16 (ties to even), as fp32 bits.  +-Inf stay, a finite value above the largest
// bf16 becomes Inf, NaN stays a quiet NaN (with its sign), -0 and subnormals as bf16 has them.  For every non-NaN
// value this is what torch's v.to(torch.bfloat16).to(torch.float32) gives on the CPU.
inline uint32_t round_bits_to_bf16(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u & 0xffff0000u) | 0x00400000u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
}

// Allocator that leaves trivially constructible elements uninitialised: a packed stream of hundreds of MB is
// written exactly once by the packers' parallel loops -- value-initialising it first walked every page on ONE core (1.8 of the
// packer's 2.2 s in the build container, where a page fault is expensive), now the copying threads touch the pages.
template <class T> struct DefaultInitAllocator : std::allocator<T> {
    template <class U> struct rebind { using other = DefaultInitAllocator<U>; };
    template <class U> void construct(U* p) noexcept { ::new ((void*)p) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};


}  // namespace hispmv
