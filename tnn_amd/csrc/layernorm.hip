// LayerNorm row kernels (reference src/nn/layers_impl/cuda/layer_norm_ops.cu
// :21 fwd, :51 bwd + the cuDNN-fe path). One block per row; fp32 stats;
// dgamma/dbeta via fp32 atomics (grid is the row count).

#include "common.h"
#include "kernels.h"

namespace tnn {


// dual block reduce: both sums in one LDS round trip
DEV void block_reduce_sum2(float& a, float& b, float* scratch16) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if (lane == 0) {
    scratch16[wid] = a;
    scratch16[8 + wid] = b;
  }
  __syncthreads();
  const int nw = blockDim.x >> 6;
  a = (threadIdx.x < nw) ? scratch16[threadIdx.x] : 0.0f;
  b = (threadIdx.x < nw) ? scratch16[8 + threadIdx.x] : 0.0f;
  if (wid == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a += __shfl_down(a, off, 64);
      b += __shfl_down(b, off, 64);
    }
  }
}

// block-wide sum handed to EVERY thread of a 256-thread block: xor butterfly
// inside the wave, one LDS slot per wave, one barrier, then each thread adds
// the four wave sums in the same order (deterministic). Saves the second
// barrier of reduce-to-thread-0 + broadcast. `scratch4` may not be rewritten
// before the block's next barrier.
DEV float block_allreduce_sum(float v, float* scratch4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) scratch4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch4[0] + scratch4[1]) + (scratch4[2] + scratch4[3]);
}

// vectorized one-block-per-row LN fwd: x held in registers across the
// mean, centred-variance and write phases (the scalar form re-reads global
// 3x; measured 10.8us for a 6.3MB pass, ~4x roofline).
// PK = 16B packs per thread; requires cols % V == 0, cols <= PK*256*V.
template <typename T, int PK>
__launch_bounds__(256)
__global__ void k_ln_fwd_vec(const T* __restrict__ x, const float* gamma,
                             const float* beta, T* __restrict__ y,
                             float* __restrict__ mean,
                             float* __restrict__ invstd, int cols, float eps) {
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) P { T e[16 / sizeof(T)]; };
  const int64_t row = blockIdx.x;
  const T* xr = x + row * cols;
  const int npk = cols / V;
  __shared__ float scratch[8];

  P v[PK];
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < PK; ++k) {
    const int pk = threadIdx.x + k * 256;
    if (pk < npk) {
      v[k] = ((const P*)xr)[pk];
#pragma unroll
      for (int j = 0; j < V; ++j) s += VecIO<T>::to_f32(v[k].e[j]);
    }
  }
  // centred second moment from the registers: E[x^2] - mean^2 cancels to
  // nothing in fp32 once |mean| >> std
  const float m = block_allreduce_sum(s, scratch) / cols;
  float ss = 0.0f;
#pragma unroll
  for (int k = 0; k < PK; ++k) {
    const int pk = threadIdx.x + k * 256;
    if (pk < npk) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = VecIO<T>::to_f32(v[k].e[j]) - m;
        ss += d * d;
      }
    }
  }
  const float is = rsqrtf(block_allreduce_sum(ss, scratch + 4) / cols + eps);
  if (threadIdx.x == 0) {
    mean[row] = m;
    invstd[row] = is;
  }
  T* yr = y + row * cols;
#pragma unroll
  for (int k = 0; k < PK; ++k) {
    const int pk = threadIdx.x + k * 256;
    if (pk < npk) {
      P o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = pk * V + j;
        const float xhat = (VecIO<T>::to_f32(v[k].e[j]) - m) * is;
        o.e[j] = VecIO<T>::from_f32(xhat * gamma[c] + beta[c]);
      }
      ((P*)yr)[pk] = o;
    }
  }
}

template <typename T, int PK>
__launch_bounds__(256)
__global__ void k_ln_bwd_vec(const T* __restrict__ x, const T* __restrict__ dy,
                             const float* gamma, const float* mean,
                             const float* invstd, T* __restrict__ dx,
                             const T* __restrict__ resid, int cols) {
  // resid: passthrough-residual grad added into dx (the pre-LN block's
  // residual junction — fused here so autograd never runs a join add)
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) P { T e[16 / sizeof(T)]; };
  const int64_t row = blockIdx.x;
  const T* xr = x + row * cols;
  const T* dyr = dy + row * cols;
  const float m = mean[row], is = invstd[row];
  const int npk = cols / V;
  __shared__ float scratch[16];
  __shared__ float s_a, s_b;

  P vx[PK], vd[PK];
  float sa = 0.0f, sb = 0.0f;
#pragma unroll
  for (int k = 0; k < PK; ++k) {
    const int pk = threadIdx.x + k * 256;
    if (pk < npk) {
      vx[k] = ((const P*)xr)[pk];
      vd[k] = ((const P*)dyr)[pk];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float g = VecIO<T>::to_f32(vd[k].e[j]) * gamma[pk * V + j];
        const float xhat = (VecIO<T>::to_f32(vx[k].e[j]) - m) * is;
        sa += g;
        sb += g * xhat;
      }
    }
  }
  block_reduce_sum2(sa, sb, scratch);
  if (threadIdx.x == 0) {
    s_a = sa / cols;
    s_b = sb / cols;
  }
  __syncthreads();
  const float ma = s_a, mb = s_b;
  T* dxr = dx + row * cols;
  const T* rr = resid ? resid + row * cols : nullptr;
#pragma unroll
  for (int k = 0; k < PK; ++k) {
    const int pk = threadIdx.x + k * 256;
    if (pk < npk) {
      P o;
      P vr;
      if (rr) vr = ((const P*)rr)[pk];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float gy = VecIO<T>::to_f32(vd[k].e[j]);
        const float xhat = (VecIO<T>::to_f32(vx[k].e[j]) - m) * is;
        float v = is * (gy * gamma[pk * V + j] - ma - xhat * mb);
        if (rr) v += VecIO<T>::to_f32(vr.e[j]);
        o.e[j] = VecIO<T>::from_f32(v);
      }
      ((P*)dxr)[pk] = o;
    }
  }
}

template <typename T>
__global__ void k_ln_fwd(const T* __restrict__ x, const float* gamma,
                         const float* beta, T* __restrict__ y,
                         float* __restrict__ mean, float* __restrict__ invstd,
                         int cols, float eps) {
  const int64_t row = blockIdx.x;
  const T* xr = x + row * cols;
  T* yr = y + row * cols;
  __shared__ float scratch[8];
  __shared__ float s_m, s_is;

  float s = 0.0f;
  for (int c = threadIdx.x; c < cols; c += blockDim.x)
    s += VecIO<T>::to_f32(xr[c]);
  s = block_reduce_sum(s, scratch);
  if (threadIdx.x == 0) s_m = s / cols;
  __syncthreads();
  const float m = s_m;

  float v = 0.0f;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    float d = VecIO<T>::to_f32(xr[c]) - m;
    v += d * d;
  }
  __syncthreads();
  v = block_reduce_sum(v, scratch);
  if (threadIdx.x == 0) {
    s_is = rsqrtf(v / cols + eps);
    mean[row] = m;
    invstd[row] = s_is;
  }
  __syncthreads();
  const float is = s_is;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    float xhat = (VecIO<T>::to_f32(xr[c]) - m) * is;
    yr[c] = VecIO<T>::from_f32(xhat * gamma[c] + beta[c]);
  }
}

template <typename T>
__global__ void k_ln_bwd(const T* __restrict__ x, const T* __restrict__ dy,
                         const float* gamma, const float* mean,
                         const float* invstd, T* __restrict__ dx,
                         const T* __restrict__ resid,
                         float* __restrict__ dgamma, float* __restrict__ dbeta,
                         int cols) {
  const int64_t row = blockIdx.x;
  const T* xr = x + row * cols;
  const T* dyr = dy + row * cols;
  T* dxr = dx + row * cols;
  const float m = mean[row], is = invstd[row];
  __shared__ float scratch[8];
  __shared__ float s_a, s_b;

  float sa = 0.0f, sb = 0.0f;  // sum(dy*gamma), sum(dy*gamma*xhat)
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    float g = VecIO<T>::to_f32(dyr[c]) * gamma[c];
    float xhat = (VecIO<T>::to_f32(xr[c]) - m) * is;
    sa += g;
    sb += g * xhat;
  }
  sa = block_reduce_sum(sa, scratch);
  __syncthreads();
  sb = block_reduce_sum(sb, scratch);
  if (threadIdx.x == 0) {
    s_a = sa / cols;
    s_b = sb / cols;
  }
  __syncthreads();
  const float ma = s_a, mb = s_b;
  const T* rr = resid ? resid + row * cols : nullptr;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    float gy = VecIO<T>::to_f32(dyr[c]);
    float xhat = (VecIO<T>::to_f32(xr[c]) - m) * is;
    float v = is * (gy * gamma[c] - ma - xhat * mb);
    if (rr) v += VecIO<T>::to_f32(rr[c]);
    dxr[c] = VecIO<T>::from_f32(v);
    if (dgamma) {  // ragged-cols fallback; the vec column kernel is used
      atomicAdd(&dgamma[c], gy * xhat);  // when cols % V == 0
      atomicAdd(&dbeta[c], gy);
    }
  }
}

// dgamma/dbeta column sums as a separate vectorized pass: the per-row
// kernel's per-element global atomics serialized 4096 rows onto the same
// 768 addresses (measured 131us for a 19MB op). Same structure as the BN
// vec reduce but with per-ROW mean/invstd.
template <typename T>
__global__ void k_ln_bwd_col(const T* __restrict__ x, const T* __restrict__ dy,
                             const float* __restrict__ mean,
                             const float* __restrict__ invstd,
                             float* __restrict__ out, int64_t rows,
                             int cols) {
  // out: gridDim.y == 1 -> the [2, cols] dgamma|dbeta buffer (single
  // writer, no zero-init); else per-slice slabs [slice][2*cols] folded
  // by k_slab_fin (no same-address atomic serialization)
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) P { T e[16 / sizeof(T)]; };
  const int groups = cols / V;
  const int gpb = min(groups, 256);
  const int rows_per_iter = 256 / gpb;
  const int g = threadIdx.x % gpb + blockIdx.x * gpb;
  const int r_off = threadIdx.x / gpb;
  __shared__ float sh[2 * 256 * V];
  float* sh_g = sh;
  float* sh_b = sh + 256 * V;
  float sg[V] = {}, sb[V] = {};
  if (g < groups && r_off < rows_per_iter) {
    const int64_t r0 = rows * blockIdx.y / gridDim.y;
    const int64_t r1 = rows * (blockIdx.y + 1) / gridDim.y;
#pragma unroll 2
    for (int64_t r = r0 + r_off; r < r1; r += rows_per_iter) {
      const float m = mean[r], is = invstd[r];
      int64_t i = r * cols + (int64_t)g * V;
      P vy = *(const P*)&dy[i];
      P vx = *(const P*)&x[i];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float gy = VecIO<T>::to_f32(vy.e[j]);
        sg[j] += gy * (VecIO<T>::to_f32(vx.e[j]) - m) * is;
        sb[j] += gy;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sh_g[threadIdx.x * V + j] = sg[j];
    sh_b[threadIdx.x * V + j] = sb[j];
  }
  __syncthreads();
  const int cpb_total = gpb * V;
  for (int cl = threadIdx.x; cl < cpb_total; cl += 256) {
    int gl = cl / V, j = cl % V;
    float tg = 0.0f, tb = 0.0f;
    for (int r = 0; r < rows_per_iter; ++r) {
      tg += sh_g[(r * gpb + gl) * V + j];
      tb += sh_b[(r * gpb + gl) * V + j];
    }
    int c = blockIdx.x * cpb_total + cl;
    if (c >= cols) break;
    float* base = out + (int64_t)blockIdx.y * 2 * cols;
    base[c] = tg;
    base[cols + c] = tb;
  }
}

void ln_fwd_launch(DT dt, const void* x, const float* gamma, const float* beta,
                   void* y, float* mean, float* invstd, int64_t rows, int cols,
                   float eps, hipStream_t s) {
  const int V = dt == DT::F32 ? 4 : 8;
  const bool vec = cols % V == 0 && (((uintptr_t)x & 15) == 0);
  const int npk = cols / V;
#define LNF(T, PK)                                                           \
  hipLaunchKernelGGL((k_ln_fwd_vec<T, PK>), dim3(rows), dim3(256), 0, s,     \
                     (const T*)x, gamma, beta, (T*)y, mean, invstd, cols, eps)
  if (vec && npk <= 4 * 256) {
    if (dt == DT::F32) {
      if (npk <= 256) LNF(float, 1);
      else if (npk <= 512) LNF(float, 2);
      else LNF(float, 4);
    } else {
      if (npk <= 256) LNF(bf16, 1);
      else if (npk <= 512) LNF(bf16, 2);
      else LNF(bf16, 4);
    }
    return;
  }
#undef LNF
  if (dt == DT::F32)
    hipLaunchKernelGGL(k_ln_fwd<float>, dim3(rows), dim3(256), 0, s,
                       (const float*)x, gamma, beta, (float*)y, mean, invstd,
                       cols, eps);
  else
    hipLaunchKernelGGL(k_ln_fwd<bf16>, dim3(rows), dim3(256), 0, s,
                       (const bf16*)x, gamma, beta, (bf16*)y, mean, invstd,
                       cols, eps);
}

// workspace floats for the vectorized dgamma/dbeta column reduce
// ((slices+1) * 2*cols incl. finalize target); 0 = scalar fallback (the
// binding must zero dgamma/dbeta for its atomics)
int64_t ln_bwd_ws_floats(DT dt, const void* x, const void* dy, int64_t rows,
                         int cols) {
  int V = dt == DT::F32 ? 4 : 8;
  bool vec = cols % V == 0 && (((uintptr_t)x & 15) == 0) &&
             (((uintptr_t)dy & 15) == 0);
  if (!vec) return 0;
  int groups = cols / V;
  int gpb = groups < 256 ? groups : 256;
  int cblocks = (groups + gpb - 1) / gpb;
  int rows_per_iter = 256 / gpb;
  int64_t iters = (rows + rows_per_iter - 1) / rows_per_iter;
  int rslices = (int)std::min<int64_t>(
      std::max<int64_t>(512 / cblocks, 1), std::max<int64_t>(iters / 4, 1));
  return rslices > 1 ? (int64_t)rslices * 2 * cols : 0;
}

void ln_bwd_launch(DT dt, const void* x, const void* dy, const float* gamma,
                   const float* mean, const float* invstd, void* dx,
                   const void* resid, float* dgamma2, float* ws, int64_t rows,
                   int cols, hipStream_t s) {
  int V = dt == DT::F32 ? 4 : 8;
  bool vec = cols % V == 0 && (((uintptr_t)x & 15) == 0) &&
             (((uintptr_t)dy & 15) == 0);
  const int npk = cols / V;
#define LNB(T, PK)                                                           \
  hipLaunchKernelGGL((k_ln_bwd_vec<T, PK>), dim3(rows), dim3(256), 0, s,     \
                     (const T*)x, (const T*)dy, gamma, mean, invstd, (T*)dx, \
                     (const T*)resid, cols)
  if (vec && npk <= 2 * 256) {  // PK<=2: x+dy packs stay in registers
    if (dt == DT::F32) {
      if (npk <= 256) LNB(float, 1);
      else LNB(float, 2);
    } else {
      if (npk <= 256) LNB(bf16, 1);
      else LNB(bf16, 2);
    }
  } else if (dt == DT::F32)
    hipLaunchKernelGGL(k_ln_bwd<float>, dim3(rows), dim3(256), 0, s,
                       (const float*)x, (const float*)dy, gamma, mean, invstd,
                       (float*)dx, (const float*)resid,
                       vec ? nullptr : dgamma2,
                       vec ? nullptr : dgamma2 + cols, cols);
  else
    hipLaunchKernelGGL(k_ln_bwd<bf16>, dim3(rows), dim3(256), 0, s,
                       (const bf16*)x, (const bf16*)dy, gamma, mean, invstd,
                       (bf16*)dx, (const bf16*)resid,
                       vec ? nullptr : dgamma2,
                       vec ? nullptr : dgamma2 + cols, cols);
#undef LNB
  if (vec) {
    int groups = cols / V;
    int gpb = groups < 256 ? groups : 256;
    int cblocks = (groups + gpb - 1) / gpb;
    int rows_per_iter = 256 / gpb;
    int64_t iters = (rows + rows_per_iter - 1) / rows_per_iter;
    // ~512 blocks (the iters/32 cap starved 768-col reduces at 64 blocks)
    int rslices = (int)std::min<int64_t>(
        std::max<int64_t>(512 / cblocks, 1), std::max<int64_t>(iters / 4, 1));
    dim3 grid(cblocks, rslices);
    float* target = rslices > 1 ? ws : dgamma2;
    if (dt == DT::F32)
      hipLaunchKernelGGL(k_ln_bwd_col<float>, grid, dim3(256), 0, s,
                         (const float*)x, (const float*)dy, mean, invstd,
                         target, rows, cols);
    else
      hipLaunchKernelGGL(k_ln_bwd_col<bf16>, grid, dim3(256), 0, s,
                         (const bf16*)x, (const bf16*)dy, mean, invstd,
                         target, rows, cols);
    if (rslices > 1) slab_fin_launch(ws, dgamma2, rslices, 2 * cols, s);
  }
}

}  // namespace tnn
