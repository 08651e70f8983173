// Region-limited edits (chronoedit_amd/region.py): the passes that keep the source outside a caller-given mask.
//
//   ce_region_weights_u8   uint8 mask [H][W] -> fp32 [H/8][W/8]: the 8x8 box mean, w = float(sum of the 64 bytes) / 16320.0f.  The sum is an
//                          integer (exact in any order), the division one correctly rounded fp32 operation: all-255 gives exactly 1.0f.
//   ce_region_blend_f32    after a scheduler step, in place on the latents:  k = (1 - s) * z_src + s * eps,  x = w * x + (1 - w) * k  with
//                          s = *sigma_next read from device memory (the loop stages it per step; a captured graph serves every step).
//   ce_region_composite    after the decode:  m = float(mask) / 255.0f,  out = m * v + (1 - m) * src  into a new fp32 video.
//
// Every `*`, `+`, `-` above is an fp32 operation rounded on its own, as the eager torch expression rounds it - hipcc contracts a * b + c
// into one fma by default, hence `#pragma clang fp contract(off)` in the two arithmetic helpers (the device of csrc/ce_image.hip's
// video_u8).  So w == 1 leaves x bit-unchanged (1 * x + 0 * k), w == 0 gives exactly k, and s == 0 gives k == z_src.
//
// All three are HBM passes with no reuse: a lane owns 16 bytes of the widest stream (four fp32 latents, eight bf16 / four fp32 video
// elements, sixteen mask bytes) when the geometry keeps every access aligned - a launch-uniform choice - and runs element by element
// otherwise.  No scratch, no state, nothing allocated: capturable.
#include "ce_common.h"

__device__ __forceinline__ uint32_t region_sum4(uint32_t v) { return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24); }

// One lane per 8x8 tile, or - WIDE (W % 16 == 0, mask 16-byte and w 8-byte aligned) - per two neighbouring tiles: one 16-byte load per
// mask row.  Lanes of a wave read one contiguous run of each of the eight rows.
template <bool WIDE>
__global__ __launch_bounds__(256) void region_weights_kernel(const uint8_t* __restrict__ mask, float* __restrict__ w, int h, int wl, int W) {
  constexpr int PER = WIDE ? 2 : 1;
  const int gpr = wl / PER;  // groups per row of tiles (WIDE: wl is even)
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)h * gpr) return;
  const int ty = (int)(g / gpr), tx = (int)(g - (long long)ty * gpr) * PER;
  const uint8_t* s = mask + ((size_t)ty * 8) * W + (size_t)tx * 8;
  float* d = w + (size_t)ty * wl + tx;
  if (WIDE) {
    uint32_t s0 = 0, s1 = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const u32x4 v = *(const u32x4*)(s + (size_t)r * W);
      s0 += region_sum4(v[0]) + region_sum4(v[1]);
      s1 += region_sum4(v[2]) + region_sum4(v[3]);
    }
    const u32x2 o = {__float_as_uint((float)s0 / 16320.0f), __float_as_uint((float)s1 / 16320.0f)};
    *(u32x2*)d = o;
  } else {
    uint32_t s0 = 0;
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) s0 += s[(size_t)r * W + c];
    d[0] = (float)s0 / 16320.0f;
  }
}

CE_API int ce_region_weights_u8(const void* mask, float* w, int H, int W, hipStream_t stream) {
  if (!mask || !w || H <= 0 || W <= 0 || H % 8 || W % 8) return CE_ERR_ARG;
  if ((long long)H * W >= (1ll << 31)) return CE_ERR_SHAPE;
  if ((uintptr_t)w & 3) return CE_ERR_ALIGN;
  const int h = H / 8, wl = W / 8;
  if (W % 16 == 0 && !((uintptr_t)mask & 15) && !((uintptr_t)w & 7)) {
    const long long groups = (long long)h * (wl / 2);
    hipLaunchKernelGGL(region_weights_kernel<true>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)mask, w, h, wl, W);
  } else {
    const long long groups = (long long)h * wl;
    hipLaunchKernelGGL(region_weights_kernel<false>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)mask, w, h, wl, W);
  }
  return (int)hipGetLastError();
}

// x_new = w * x + (1 - w) * ((1 - s) * z + s * e): seven fp32 roundings (oms = 1 - s is formed once per launch, the same operation).
// bf16_out: the "reference-precision trajectory" of the step kernel (flags & 2) - the stored sample carries a bf16 value.
__device__ __forceinline__ float region_blend1(float x, float z, float e, float w, float s, float oms, bool bf16_out) {
#pragma clang fp contract(off)
  const float a = oms * z;
  const float b = s * e;
  const float k = a + b;
  const float c = w * x;
  const float omw = 1.0f - w;
  const float d = omw * k;
  const float r = c + d;
  return bf16_out ? round_bf16(r) : r;
}

__device__ __forceinline__ float region_one_minus(float s) {
#pragma clang fp contract(off)
  return 1.0f - s;
}

// Grid-stride over groups of four elements (WIDE: plane % 4 == 0 and x, z_src, eps, w 16-byte aligned, so a group lies in one plane and
// every access is one aligned vector) or over single elements.  w is indexed by the position inside the h*w plane: broadcast over
// batch, channel and frame.
template <bool WIDE>
__global__ __launch_bounds__(256) void region_blend_kernel(float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ e,
                                                           const float* __restrict__ w, const float* __restrict__ sigma_next, long long n,
                                                           long long plane, int flags) {
  const float s = sigma_next[0], oms = region_one_minus(s);
  const bool bf16_out = (flags & 2) != 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (WIDE) {
    const long long groups = n >> 2;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
      const long long i = g << 2;
      const u32x4 xv = *(const u32x4*)(x + i), zv = *(const u32x4*)(z + i), ev = *(const u32x4*)(e + i);
      const u32x4 wv = *(const u32x4*)(w + i % plane);
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = __float_as_uint(region_blend1(__uint_as_float(xv[j]), __uint_as_float(zv[j]), __uint_as_float(ev[j]), __uint_as_float(wv[j]), s, oms, bf16_out));
      *(u32x4*)(x + i) = o;
    }
  } else {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
      x[i] = region_blend1(x[i], z[i], e[i], w[i % plane], s, oms, bf16_out);
  }
}

// the block cap of the step kernel this pass follows (csrc/ce_sched.hip cfg_unipc_blocks)
static unsigned region_blend_blocks(long long work) {
  const long long blocks = (work + 255) / 256;
  return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

CE_API int ce_region_blend_f32(float* x, const float* z_src, const float* eps, const float* w, const float* sigma_next, long long n,
                               long long plane, int flags, hipStream_t stream) {
  if (!x || !z_src || !eps || !w || !sigma_next || n <= 0 || plane <= 0 || n % plane) return CE_ERR_ARG;
  const uintptr_t all = (uintptr_t)x | (uintptr_t)z_src | (uintptr_t)eps | (uintptr_t)w;
  if ((all | (uintptr_t)sigma_next) & 3) return CE_ERR_ALIGN;
  if (plane % 4 == 0 && !(all & 15))
    hipLaunchKernelGGL(region_blend_kernel<true>, dim3(region_blend_blocks(n / 4)), dim3(256), 0, stream, x, z_src, eps, w, sigma_next, n, plane, flags);
  else
    hipLaunchKernelGGL(region_blend_kernel<false>, dim3(region_blend_blocks(n)), dim3(256), 0, stream, x, z_src, eps, w, sigma_next, n, plane, flags);
  return (int)hipGetLastError();
}

// out = m * v + (1 - m) * src with m = float(byte) / 255.0f: a division, a subtraction, two multiplies and an add, each rounded in fp32.
__device__ __forceinline__ float region_paste1(float v, float src, uint32_t byte) {
#pragma clang fp contract(off)
  const float m = (float)byte / 255.0f;
  const float a = m * v;
  const float omm = 1.0f - m;
  const float b = omm * src;
  return a + b;
}

__device__ __forceinline__ float region_elem(const uint16_t* p, size_t i) { return bf16_bits_to_f32(p[i]); }
__device__ __forceinline__ float region_elem(const float* p, size_t i) { return p[i]; }

// One lane per P = 16 / sizeof(T) consecutive pixels of one (sample, channel, frame) plane of the video: 16 bytes of v, 2 P bytes of the
// bf16 source plane (sample, channel), P mask bytes, 4 P bytes of output.  WIDE (H W % P == 0, v and out 16-byte, src 2 P-byte and mask
// P-byte aligned): every access is one aligned vector; otherwise element by element with a tail in the last group of a plane.
template <typename T, bool WIDE>
__global__ __launch_bounds__(256) void region_composite_kernel(const T* __restrict__ v, const uint16_t* __restrict__ src, const uint8_t* __restrict__ mask,
                                                               float* __restrict__ out, int F, long long hw, long long planes) {
  constexpr int P = 16 / (int)sizeof(T);
  const long long gpp = (hw + P - 1) / P;  // groups per plane
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= planes * gpp) return;
  const long long pl = g / gpp, p0 = (g - pl * gpp) * P;  // pl = (b * 3 + c) * F + f
  const long long bc = pl / F;                            // b * 3 + c: the source plane
  const T* vs = v + (size_t)pl * hw + p0;
  const uint16_t* ss = src + (size_t)bc * hw + p0;
  const uint8_t* ms = mask + p0;
  float* d = out + (size_t)pl * hw + p0;
  if (WIDE) {
    float vf[P], sf[P];
    uint32_t mb[P];
    const u32x4 vv = *(const u32x4*)vs;
    if constexpr (sizeof(T) == 2) {
      const u32x4 sv = *(const u32x4*)ss;
      const u32x2 mv = *(const u32x2*)ms;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        vf[2 * k] = bf16lo(vv[k]), vf[2 * k + 1] = bf16hi(vv[k]);
        sf[2 * k] = bf16lo(sv[k]), sf[2 * k + 1] = bf16hi(sv[k]);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) mb[k] = (mv[k >> 2] >> (8 * (k & 3))) & 255u;
    } else {
      const u32x2 sv = *(const u32x2*)ss;
      const uint32_t mv = *(const uint32_t*)ms;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        vf[k] = __uint_as_float(vv[k]);
        mb[k] = (mv >> (8 * k)) & 255u;
      }
      sf[0] = bf16lo(sv[0]), sf[1] = bf16hi(sv[0]), sf[2] = bf16lo(sv[1]), sf[3] = bf16hi(sv[1]);
    }
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __float_as_uint(region_paste1(vf[4 * q + j], sf[4 * q + j], mb[4 * q + j]));
      *(u32x4*)(d + 4 * q) = o;
    }
  } else {
    const int npx = (int)((hw - p0) < P ? (hw - p0) : P);
    for (int i = 0; i < npx; ++i) d[i] = region_paste1(region_elem(vs, i), bf16_bits_to_f32(ss[i]), ms[i]);
  }
}

template <typename T>
static int region_composite_launch(const void* v, const void* src, const void* mask, float* out, int B, int F, long long hw, hipStream_t stream) {
  constexpr int P = 16 / (int)sizeof(T);
  const long long planes = (long long)B * 3 * F, groups = planes * ((hw + P - 1) / P);
  if (groups > 0x7fffffffll * 256) return CE_ERR_SHAPE;
  const dim3 grid((unsigned)((groups + 255) / 256));
  const bool wide = hw % P == 0 && !(((uintptr_t)v | (uintptr_t)out) & 15) && !((uintptr_t)src & (2 * P - 1)) && !((uintptr_t)mask & (P - 1));
  if (wide)
    hipLaunchKernelGGL((region_composite_kernel<T, true>), grid, dim3(256), 0, stream, (const T*)v, (const uint16_t*)src, (const uint8_t*)mask, out, F, hw, planes);
  else
    hipLaunchKernelGGL((region_composite_kernel<T, false>), grid, dim3(256), 0, stream, (const T*)v, (const uint16_t*)src, (const uint8_t*)mask, out, F, hw, planes);
  return (int)hipGetLastError();
}

CE_API int ce_region_composite(const void* v, int v_is_bf16, const void* src, const void* mask, float* out, int B, int F, int H, int W,
                               hipStream_t stream) {
  if (!v || !src || !mask || !out || v == (const void*)out || B <= 0 || F <= 0 || H <= 0 || W <= 0) return CE_ERR_ARG;
  if (((uintptr_t)v & (v_is_bf16 ? 1 : 3)) || ((uintptr_t)src & 1) || ((uintptr_t)out & 3)) return CE_ERR_ALIGN;
  const long long hw = (long long)H * W;
  return v_is_bf16 ? region_composite_launch<uint16_t>(v, src, mask, out, B, F, hw, stream)
                   : region_composite_launch<float>(v, src, mask, out, B, F, hw, stream);
}
