// Fused optimizer update kernels (reference sgd_kernels.cu:17,26,
// adam_kernels.cu:19,56). One pass: read grad (any dtype), update fp32
// master + moments, write the low-precision parameter — the mixed-precision
// upgrade over the reference's fp32-only updates.
//
// Global-norm gradient clipping is fused in: k_gradsq_mt writes one fp32
// sum-of-squares partial per MT_CHUNK span, k_clip_fin folds them in a
// fixed order into a small fp32 state vector (CLIP_* slots in kernels.h),
// and the update kernels read the coefficient and the skip flag from that
// vector. They likewise read the learning rate from device memory when
// handed `lr_dev`, so a hipGraph-captured step follows a scheduler. Both
// pointers null = the code path without clipping.

#include "common.h"
#include "kernels.h"

namespace tnn {

template <typename TP, typename TG>
__global__ void k_sgd(TP* __restrict__ p, float* __restrict__ master,
                      const TG* __restrict__ g, float* __restrict__ buf,
                      int64_t n, float lr, float momentum, float wd,
                      bool nesterov, bool has_master,
                      const float* __restrict__ clip,
                      const float* __restrict__ lr_dev) {
  // non-finite global norm: param, master and momentum stay untouched
  // (coef * inf is not 0, so this has to be an exit, not a scale)
  if (clip && clip[CLIP_SKIP] != 0.0f) return;
  const float coef = clip ? clip[CLIP_COEF] : 1.0f;
  if (lr_dev) lr = *lr_dev;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float w = has_master ? master[i] : VecIO<TP>::to_f32(p[i]);
    float gr = VecIO<TG>::to_f32(g[i]);
    if (clip) gr *= coef;
    gr += wd * w;
    if (buf) {
      float b = buf[i] * momentum + gr;
      buf[i] = b;
      gr = nesterov ? gr + momentum * b : b;
    }
    w -= lr * gr;
    if (has_master) master[i] = w;
    p[i] = VecIO<TP>::from_f32(w);
  }
}

template <typename TP, typename TG>
__global__ void k_adam(TP* __restrict__ p, float* __restrict__ master,
                       const TG* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, int64_t n, float lr, float beta1,
                       float beta2, float eps, float wd, float bc1, float bc2,
                       bool adamw, bool has_master,
                       const int64_t* __restrict__ step_dev,
                       const float* __restrict__ clip,
                       const float* __restrict__ lr_dev) {
  if (clip && clip[CLIP_SKIP] != 0.0f) return;  // see k_sgd
  const float coef = clip ? clip[CLIP_COEF] : 1.0f;
  if (lr_dev) lr = *lr_dev;
  if (step_dev) {
    // hipGraph-captured step: bias correction from the device step
    // counter (incremented in-graph), not a baked-in host value
    const float t = (float)*step_dev;
    bc1 = 1.0f - powf(beta1, t);  // precise powf: bitwise-matches the
    bc2 = 1.0f - powf(beta2, t);  // host-computed eager bias correction
  }
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float w = has_master ? master[i] : VecIO<TP>::to_f32(p[i]);
    float gr = VecIO<TG>::to_f32(g[i]);
    if (clip) gr *= coef;
    if (!adamw) gr += wd * w;
    float mi = m[i] = beta1 * m[i] + (1.0f - beta1) * gr;
    float vi = v[i] = beta2 * v[i] + (1.0f - beta2) * gr * gr;
    if (adamw) w *= (1.0f - lr * wd);
    w -= lr / bc1 * mi / (sqrtf(vi / bc2) + eps);
    if (has_master) master[i] = w;
    p[i] = VecIO<TP>::from_f32(w);
  }
}

// Multi-tensor Adam: one launch for a whole parameter group. desc holds
// 6 int64 per tensor (param, master, grad, m, v pointers + numel); chunks
// maps each block to (tensor_idx << 32 | chunk_index) over CHUNK-element
// spans. Collapses ~150 per-parameter launches into one.
constexpr int MT_CHUNK = 16384;

template <typename TP, typename TG, bool MASTER>
__launch_bounds__(256)
__global__ void k_adam_mt(const int64_t* __restrict__ desc,
                          const int64_t* __restrict__ chunks, float lr,
                          float beta1, float beta2, float eps, float wd,
                          float bc1, float bc2, bool adamw,
                          const int64_t* __restrict__ step_dev,
                          const float* __restrict__ clip,
                          const float* __restrict__ lr_dev) {
  if (clip && clip[CLIP_SKIP] != 0.0f) return;  // see k_sgd
  const float coef = clip ? clip[CLIP_COEF] : 1.0f;
  if (lr_dev) lr = *lr_dev;
  if (step_dev) {
    const float t = (float)*step_dev;
    bc1 = 1.0f - powf(beta1, t);  // precise powf (see k_adam)
    bc2 = 1.0f - powf(beta2, t);
  }
  int64_t c = chunks[blockIdx.x];
  int ti = (int)(c >> 32);
  int64_t off = (int64_t)(c & 0xffffffff) * MT_CHUNK;
  const int64_t* d = desc + (int64_t)ti * 6;
  TP* p = (TP*)d[0];
  float* master = (float*)d[1];
  const TG* g = (const TG*)d[2];
  float* m = (float*)d[3];
  float* v = (float*)d[4];
  int64_t n = d[5];
  int64_t end = off + MT_CHUNK < n ? off + MT_CHUNK : n;
  // 4-wide vector path: m/v/master float4, p/g 4-element packs (the
  // scalar loop measured ~1.5x off the update's memory roofline)
  struct alignas(4 * sizeof(TP)) P4 { TP e[4]; };
  struct alignas(4 * sizeof(TG)) G4 { TG e[4]; };
  const bool vec4 = (end - off) % 4 == 0 && ((uintptr_t)p & 15) == 0 &&
                    ((uintptr_t)g & 15) == 0;
  if (vec4) {
    // 2-deep unroll: two independent float4 groups' loads in flight per
    // thread (the single-group loop measured 4.3 TB/s on the 5-stream
    // read/write mix)
#pragma unroll 2
    for (int64_t i4 = off / 4 + threadIdx.x; i4 * 4 < end; i4 += 256) {
      float4 mi4 = ((float4*)m)[i4];
      float4 vi4 = ((float4*)v)[i4];
      float4 w4;
      if (MASTER) w4 = ((float4*)master)[i4];
      P4 pp;
      if (!MASTER) pp = ((P4*)p)[i4];
      G4 gg = ((const G4*)g)[i4];
      float* wv = (float*)&w4;
      float* mv = (float*)&mi4;
      float* vv = (float*)&vi4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float w = MASTER ? wv[j] : VecIO<TP>::to_f32(pp.e[j]);
        float gr = VecIO<TG>::to_f32(gg.e[j]);
        if (clip) gr *= coef;
        if (!adamw) gr += wd * w;
        float mi = mv[j] = beta1 * mv[j] + (1.0f - beta1) * gr;
        float vi = vv[j] = beta2 * vv[j] + (1.0f - beta2) * gr * gr;
        if (adamw) w *= (1.0f - lr * wd);
        w -= lr / bc1 * mi / (sqrtf(vi / bc2) + eps);
        wv[j] = w;
        pp.e[j] = VecIO<TP>::from_f32(w);
      }
      ((float4*)m)[i4] = mi4;
      ((float4*)v)[i4] = vi4;
      if (MASTER) ((float4*)master)[i4] = w4;
      ((P4*)p)[i4] = pp;
    }
    return;
  }
  for (int64_t i = off + threadIdx.x; i < end; i += 256) {
    float w = MASTER ? master[i] : VecIO<TP>::to_f32(p[i]);
    float gr = VecIO<TG>::to_f32(g[i]);
    if (clip) gr *= coef;
    if (!adamw) gr += wd * w;
    float mi = m[i] = beta1 * m[i] + (1.0f - beta1) * gr;
    float vi = v[i] = beta2 * v[i] + (1.0f - beta2) * gr * gr;
    if (adamw) w *= (1.0f - lr * wd);
    w -= lr / bc1 * mi / (sqrtf(vi / bc2) + eps);
    if (MASTER) master[i] = w;
    p[i] = VecIO<TP>::from_f32(w);
  }
}

// ---- global gradient norm --------------------------------------------------
// 16-byte pack of gradients -> fp32 sum of squares, added in element order.
template <typename TG> struct GradPack;
template <> struct GradPack<float> { using V = float4; };
template <> struct GradPack<bf16> { using V = uint4; };

DEV float sumsq_pack(float4 x, float acc) {
  acc = fmaf(x.x, x.x, acc);
  acc = fmaf(x.y, x.y, acc);
  acc = fmaf(x.z, x.z, acc);
  return fmaf(x.w, x.w, acc);
}
DEV float sumsq_pack(uint4 x, float acc) {  // 8 bf16: low half = even element
  const unsigned int u[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float lo = __uint_as_float(u[j] << 16);
    const float hi = __uint_as_float(u[j] & 0xffff0000u);
    acc = fmaf(lo, lo, acc);
    acc = fmaf(hi, hi, acc);
  }
  return acc;
}

// Multi-tensor sum of squares, same launch shape as k_adam_mt: block b
// covers one MT_CHUNK span of one tensor and writes ONE fp32 partial to
// part[b]. No atomics — k_clip_fin folds the partials in a fixed order, so
// the norm is bitwise reproducible. The descriptor is `stride` int64 per
// tensor with the grad pointer in slot `gslot` and numel in slot `nslot`
// (k_adam_mt's 6-wide descriptor is read as it is: stride 6, slots 2, 5).
// Each thread chains at most MT_CHUNK/256 = 64 fp32 fmas.
template <typename TG>
__launch_bounds__(256)
__global__ void k_gradsq_mt(const int64_t* __restrict__ desc,
                            const int64_t* __restrict__ chunks, int stride,
                            int gslot, int nslot, float* __restrict__ part) {
  __shared__ float red[256 / WAVE];
  const int64_t c = chunks[blockIdx.x];
  const int ti = (int)(c >> 32);
  const int64_t off = (int64_t)(c & 0xffffffff) * MT_CHUNK;
  const int64_t* d = desc + (int64_t)ti * stride;
  const TG* g = (const TG*)d[gslot];
  const int64_t n = d[nslot];
  const int64_t end = off + MT_CHUNK < n ? off + MT_CHUNK : n;
  constexpr int PACK = 16 / sizeof(TG);
  float acc = 0.0f;
  // grads may be views into a packed slab at any element offset, so the
  // span start is tested, not the tensor base
  // Both forms issue a group of independent loads before the first fma
  // (one load per trip left the kernel latency-bound) and add in index
  // order, so the sum does not depend on the grouping.
  if ((end - off) % PACK == 0 && ((uintptr_t)(g + off) & 15) == 0) {
    using V = typename GradPack<TG>::V;
    const V* gv = (const V*)(g + off);
    const int np = (int)((end - off) / PACK);
    int k = threadIdx.x;
    for (; k + 3 * 256 < np; k += 4 * 256) {
      const V a = gv[k], b = gv[k + 256], c2 = gv[k + 512], e = gv[k + 768];
      acc = sumsq_pack(a, acc);
      acc = sumsq_pack(b, acc);
      acc = sumsq_pack(c2, acc);
      acc = sumsq_pack(e, acc);
    }
    for (; k < np; k += 256) acc = sumsq_pack(gv[k], acc);
  } else {
    int64_t i = off + threadIdx.x;
    for (; i + 7 * 256 < end; i += 8 * 256) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = VecIO<TG>::to_f32(g[i + j * 256]);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf(x[j], x[j], acc);
    }
    for (; i < end; i += 256) {
      const float x = VecIO<TG>::to_f32(g[i]);
      acc = fmaf(x, x, acc);
    }
  }
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One block: fold the partials of every k_gradsq_mt launch of this step
// (thread t takes t, t+256, ... in double, then a fixed tree), or take an
// already reduced `sumsq_in` (sum over ranks), and derive the clip state.
// `sumsq_in` may alias state + CLIP_SUMSQ. `skipped` (nullable) counts the
// steps whose norm was not finite.
__launch_bounds__(256)
__global__ void k_clip_fin(const float* part, int npart,
                           const float* sumsq_in, float max_norm,
                           float* state, int64_t* skipped) {
  __shared__ double sh[256];
  float sumsq;
  if (sumsq_in) {
    sumsq = *sumsq_in;
  } else {
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) acc += (double)part[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
      __syncthreads();
    }
    sumsq = (float)sh[0];
  }
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(sumsq);
  const bool skip = !isfinite(norm);
  // torch.nn.utils.clip_grad_norm_'s rule
  const float coef =
      max_norm > 0.0f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
  state[CLIP_SUMSQ] = sumsq;
  state[CLIP_NORM] = norm;
  state[CLIP_COEF] = coef;
  state[CLIP_SKIP] = skip ? 1.0f : 0.0f;
  if (skip && skipped) *skipped += 1;
}

void grad_sumsq_mt_launch(DT dt_g, const int64_t* desc, const int64_t* chunks,
                          int nchunks, int stride, int gslot, int nslot,
                          float* part, hipStream_t s) {
  if (nchunks <= 0) return;
  if (dt_g == DT::F32)
    hipLaunchKernelGGL((k_gradsq_mt<float>), dim3(nchunks), dim3(256), 0, s,
                       desc, chunks, stride, gslot, nslot, part);
  else
    hipLaunchKernelGGL((k_gradsq_mt<bf16>), dim3(nchunks), dim3(256), 0, s,
                       desc, chunks, stride, gslot, nslot, part);
}

void clip_finalize_launch(const float* part, int npart, const float* sumsq_in,
                          float max_norm, float* state, int64_t* skipped,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_clip_fin, dim3(1), dim3(256), 0, s, part, npart,
                     sumsq_in, max_norm, state, skipped);
}

void adam_mt_launch(DT dt_p, DT dt_g, bool has_master, const int64_t* desc,
                    const int64_t* chunks, int nchunks, int step,
                    const int64_t* step_dev, float lr, float beta1,
                    float beta2, float eps, float weight_decay, bool adamw,
                    const float* clip, const float* lr_dev, hipStream_t s) {
  float bc1 = 1.0f - powf(beta1, (float)step);
  float bc2 = 1.0f - powf(beta2, (float)step);
#define CASE(TP, TG, M)                                                      \
  hipLaunchKernelGGL((k_adam_mt<TP, TG, M>), dim3(nchunks), dim3(256), 0, s, \
                     desc, chunks, lr, beta1, beta2, eps, weight_decay, bc1, \
                     bc2, adamw, step_dev, clip, lr_dev)
  if (has_master) {
    if (dt_p == DT::F32 && dt_g == DT::F32) CASE(float, float, true);
    else if (dt_p == DT::BF16 && dt_g == DT::BF16) CASE(bf16, bf16, true);
    else if (dt_p == DT::BF16 && dt_g == DT::F32) CASE(bf16, float, true);
    else CASE(float, bf16, true);
  } else {
    if (dt_p == DT::F32 && dt_g == DT::F32) CASE(float, float, false);
    else if (dt_p == DT::BF16 && dt_g == DT::BF16) CASE(bf16, bf16, false);
    else if (dt_p == DT::BF16 && dt_g == DT::F32) CASE(bf16, float, false);
    else CASE(float, bf16, false);
  }
#undef CASE
}

static inline int ob(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 2048 ? b : 2048);
}

void sgd_step_launch(DT dt_p, const void* grad, DT dt_g, void* param,
                     float* master, float* momentum_buf, int64_t n, float lr,
                     float momentum, float weight_decay, bool nesterov,
                     bool has_master, const float* clip, const float* lr_dev,
                     hipStream_t s) {
#define CASE(TP, TG)                                                          \
  hipLaunchKernelGGL((k_sgd<TP, TG>), dim3(ob(n)), dim3(256), 0, s,           \
                     (TP*)param, master, (const TG*)grad, momentum_buf, n,    \
                     lr, momentum, weight_decay, nesterov, has_master, clip,  \
                     lr_dev)
  if (dt_p == DT::F32 && dt_g == DT::F32) CASE(float, float);
  else if (dt_p == DT::BF16 && dt_g == DT::BF16) CASE(bf16, bf16);
  else if (dt_p == DT::BF16 && dt_g == DT::F32) CASE(bf16, float);
  else CASE(float, bf16);
#undef CASE
}

void adam_step_launch(DT dt_p, const void* grad, DT dt_g, void* param,
                      float* master, float* m, float* v, int64_t n, int step,
                      const int64_t* step_dev, float lr, float beta1,
                      float beta2, float eps, float weight_decay, bool adamw,
                      bool has_master, const float* clip, const float* lr_dev,
                      hipStream_t s) {
  float bc1 = 1.0f - powf(beta1, (float)step);
  float bc2 = 1.0f - powf(beta2, (float)step);
#define CASE(TP, TG)                                                          \
  hipLaunchKernelGGL((k_adam<TP, TG>), dim3(ob(n)), dim3(256), 0, s,          \
                     (TP*)param, master, (const TG*)grad, m, v, n, lr, beta1, \
                     beta2, eps, weight_decay, bc1, bc2, adamw, has_master,   \
                     step_dev, clip, lr_dev)
  if (dt_p == DT::F32 && dt_g == DT::F32) CASE(float, float);
  else if (dt_p == DT::BF16 && dt_g == DT::BF16) CASE(bf16, bf16);
  else if (dt_p == DT::BF16 && dt_g == DT::F32) CASE(bf16, float);
  else CASE(float, bf16);
#undef CASE
}

}  // namespace tnn

