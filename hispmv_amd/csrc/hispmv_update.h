// hispmv_update.h -- in-place value updates of loaded handles (hispmv_update_values*, include/hispmv.h): the device side.
// A handle created with value updates on carries a MAP: for every value slot of its device layouts, in chunks of kValueChunk
// slots, the position k + 1 of the creation input entry the slot holds (0 = filler / padding).  An update gathers the new values
// through it into the layouts, in place (hispmv_update.hip).  Kept apart from hispmv_kernels.hip, whose step kernel sits at its
// register ceiling.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hispmv {

constexpr int kValueChunk = 1024;     // slots per chunk: one slice's values (slice stream) or one 1024-word slice (tile stream)

// One chunk of the map: slots [map_off, map_off + kValueChunk) of the map go to dst0 and, when not NULL, to dst1 (the batch
// layout's copy of the same slice).  Both 16-byte aligned.
// bf16 handles: a destination is kValueChunk fp32 slots as above or a HALF slice (hispmv_format.h), whose values are the first 8 bytes
// of each 16-byte piece.  The kinds ride in the two low bits of map_off (a multiple of kValueChunk): the struct, which is charged to
// the arena, and the tables of fp32 handles stay as they were.  Only the bf16 kernels look at the bits; fp32 handles never set them.
constexpr int64_t kChunkHalf0 = 1, kChunkHalf1 = 2;      // map_off bits: dst0 / dst1 is a half slice
struct ValueChunkDev {
    int64_t map_off;
    float* dst0;
    float* dst1;
};

// map[chunk] = the payloads the creation left in the chunk's first destination (bits of k + 1, or 0), for every chunk of the table.
hipError_t launch_build_value_map(const ValueChunkDev* d_table, int64_t n_chunks, int32_t* d_map, hipStream_t s);
// dst[slot] = map[slot] ? values[map[slot] - 1] : 0 for every chunk of the table (an index above n also writes 0).
hipError_t launch_update_values(const ValueChunkDev* d_table, int64_t n_chunks, const int32_t* d_map, const float* d_values, int64_t n,
                                hipStream_t s);
// bf16 handles: the same gather, every value rounded on the device to the nearest bfloat16 -- bit for bit round_bits_to_bf16
// (hispmv_format.h) -- and stored by the destination's kind: R(v) as fp32 bits into 32-bit slots, its upper half into the value halves
// of a half slice ({v0 | v1 << 16, v2 | v3 << 16} at dst + 16 * t for the 4 elements of thread t; bytes 8..15, the metas, untouched).
hipError_t launch_update_values_bf16(const ValueChunkDev* d_table, int64_t n_chunks, const int32_t* d_map, const float* d_values, int64_t n,
                                     hipStream_t s);
// Dense bf16 W (rows x cols row-major, 2 bytes per element): dst[i] = upper half of R(src[i]) for i < n.
hipError_t launch_update_dense_bf16(uint16_t* d_dst, const float* d_src, int64_t n, hipStream_t s);

}  // namespace hispmv
