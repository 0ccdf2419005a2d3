// Gather flash-attention forward with INT8 SCORES and e4m3 P V (include/vorta_hip.h: vorta_attn_fwd_i8, ABI 6).
//
// Why: the score is where an 8-bit format costs.  e4m3 keeps 3 mantissa bits wherever a value sits, so a logit is off by
// 3.7 % of the root sum of squares of its 128 products (attn_fwd_fp8.hip: 40 dB against the 16-bit kernels only where the
// softmax is flat); int8 keeps 7 bits next to the operand's maximum and runs at the same MFMA rate (v_mfma_i32_32x32x32_i8:
// the cycles of the 16-bit 32x32x16 form at twice the K).  With both operands centred -- the term the query centre leaves,
// b[key] = cq . (k - ck), is exact float32 work of the quantiser (i8_quant.hip) and enters the accumulator as its initial
// value -- and their channel ranges balanced, it holds >= 40 dB on every input family of tests/_fp8_inputs.py.
//
// What an int32 accumulator must NOT cost is VALU work per score (a first version with a scale per key row -- convert,
// multiply, multiply-add, exp2, pack: five instructions per score -- ran at the mixed kernel's 1.2 x of bf16, not at the
// e4m3 kernel's 1.7 x).  Here a score costs TWO instructions between the score MFMA and the P V MFMA (round 6: 1.75 -- the
// conversions two at a time, VORTA_I8_PKNORM below):
//   * the accumulator starts from 0x4B400000 + seed[key] (the integer whose float reading is 1.5 2^23 + seed), so after the
//     MFMAs its bits READ AS A FLOAT are 1.5 2^23 + (q8 . k8 + seed), exactly: no v_cvt_f32_i32;
//   * one v_fma_f32 with the wave's unit (8 scale log2e sq sk) and an offset that folds the magic constant, the reference
//     point, p_bias and the e4m3 exponent bias gives y = 8 log2 P' + 56;
//   * one v_cvt_pk_u8_f32 writes rint(y) as the e4m3 BYTE of P' (exponent field = integer part of log2 P', mantissa = linear
//     interpolation of its fraction: +-3 % of 2^x, ~0.5-0.8 dB of output PSNR) straight into the B operand of the P V MFMA:
//     no v_exp_f32, no v_cvt_pk_fp8_f32.
// Scales are uniform where the MFMA needs them uniform: one key scale per head (sk), one query scale per WAVE (sq, taken by
// the wave itself over its 32 rows -- queries are read once per workgroup).  The per-key seeds depend on the wave's sq:
// every wave turns the block's 64 float biases (LDS-DMA'd with the K tile, one step further ahead) into integers with three
// VALU instructions, parks them in a private 256-byte LDS slot and reads them back as the accumulators' initial values.
//
// Structure otherwise: K tile int8 rows of 128 bytes (8 KiB, the e4m3 kernels' image), V tile e4m3 through ds_read_b64_tr_b8,
// O^T += V8^T P'^T on v_mfma_f32_32x32x64_f8f6f4, row sums from the ones-tile MFMA, deferred rescale, v_descale in the
// epilogue; the loop is the e4m3 kernel's (attn_fwd_fp8.hip): the two waves of a SIMD take turns between a matrix part (13
// MFMAs: per wave and 64-key block 8 of 32 cycles + 5 of 64 = 576 pipe cycles; 1 024 in 16 bits, 832 mixed, 576 all-e4m3)
// and a VALU part.  What bounds it is the SIMD's vector issue: ~92 VALU instructions of ~5.4 cycles and 13 MFMA issues of 8
// per wave and block, two waves = ~1 200 cycles of issue beside 1 152 of matrix pipe, plus the tile requests (~90 cycles
// of the issuing wave each, wherever they stand) and the barrier: tools/trace_i8.py measures ~1 600 cycles per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"

#include "attn_i8_body.h"

namespace {
using namespace vorta_attn;

template <typename T, int NW, bool KVTAB>
__global__ __launch_bounds__(NW * 64, 2) void attn_i8_kernel(const ParamsI8 pp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[SMEM_I8];
  const int wg = live_order(pp.p, blockIdx.x, gridDim.x, pp.p.xcd_remap);  // XCD-aware order over the live workgroups
  attn_i8_body<T, NW, KVTAB, NSI8>(pp, smem, wg);
#endif
}

// Several launches fused into ONE grid (the experts of a routed layer), as attn_fwd_multi_kernel
template <typename T>
__global__ __launch_bounds__(512, 2) void attn_i8_multi_kernel(const MultiOf<ParamsI8> mp) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) char smem[SMEM_I8];
  int wg;
  const ParamsI8& pp = segment_of(mp, blockIdx.x, wg);
  if (pp.p.kv_rows) attn_i8_body<T, 8, true, NSI8>(pp, smem, wg);
  else attn_i8_body<T, 8, false, NSI8>(pp, smem, wg);
#endif
}

struct FamilyI8 {
  using PP = ParamsI8;
  const vorta_attn_i8_ext* ext;
  int fill(const vorta_attn_args* a, ParamsI8& pp, int& block_rows) const { return fill_i8(a, ext, pp, block_rows); }
  bool fusable(const vorta_attn_args&, const ParamsI8&) const { return true; }
  int out_dtype(const vorta_attn_args& a) const { return a.dtype; }
  template <typename T> static constexpr auto multi = attn_i8_multi_kernel<T>;
  template <typename T> static auto kernel(const vorta_attn_args&, const ParamsI8& pp, int block_rows) {
    if (block_rows == 256) return pp.p.kv_rows ? attn_i8_kernel<T, 8, true> : attn_i8_kernel<T, 8, false>;
    return pp.p.kv_rows ? attn_i8_kernel<T, 4, true> : attn_i8_kernel<T, 4, false>;
  }
};

}  // namespace

extern "C" int vorta_attn_fwd_i8(const vorta_attn_args* a, const vorta_attn_i8_ext* ext, void* hip_stream) {
  return fwd_single(FamilyI8{ext}, a, hip_stream);
}

extern "C" int vorta_attn_fwd_batch_i8(const vorta_attn_args* args, const vorta_attn_i8_ext* ext, int32_t n, void* hip_stream) {
  if (!ext) return VORTA_EINVAL;
  return fwd_batch(FamilyI8{ext}, args, n, hip_stream);
}
