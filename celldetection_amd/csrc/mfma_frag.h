// The fragment idiom of v_mfma_f32_32x32x16_bf16 (D[i][j] += sum over k < 16 of A[i][k] B[k][j]) with operands that lie in LDS as
// [k][32 columns] bf16, 64 bytes per row -- the reduction index is the ROW index of the operand as it lies (a pixel, in every user).
// Lane l supplies A[l % 32][8 (l / 32) + e] or B[8 (l / 32) + e][l % 32], e = 0 ... 7.  With ds_read_b64_tr_b16 a lane gives the
// address of ITS row, not of its column: of the 16 rows of a step the rows t = 8 (l / 32) + (l >> 2) % 4 and t + 4, at the byte
// offset mf_lane_bytes of four columns, and the two reads together are the lane's operand.  D: lane l holds column j = l % 32,
// register r holds row i = mf_row(r, l / 32).
// Used by csrc/wgrad_dense.h, csrc/grouped_conv_train.hip, csrc/stem_train.hip, csrc/image_conv_train.hip (and csrc/stem_mfma.h) and csrc/readout_tail.hip.
// Device code with internal linkage: every unit that includes this header gets its own copy, compiled with that unit's flags.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// the transposed 8-byte LDS read: EXEC must be all ones around it, the address a multiple of 8
__device__ __forceinline__ s16x4 mf_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

// the operand of one MFMA step from the byte offsets of the lane's two rows (t and t + 4), mf_lane_bytes included
__device__ __forceinline__ bf16x8 mf_operand(const char *smem, int row0_offset, int row1_offset) {
    const s16x4 lo = mf_read_tr(smem, row0_offset), hi = mf_read_tr(smem, row1_offset);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// byte offset of the lane's four columns inside a 64-byte row
__device__ __forceinline__ int mf_lane_bytes(int lane) { return (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2; }

// row i of D that accumulator register r holds in lane half h = lane / 32
__device__ __forceinline__ int mf_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

__device__ __forceinline__ void mf_zero(f32x16 &acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

}  // namespace
