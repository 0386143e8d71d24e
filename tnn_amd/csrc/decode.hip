// Fused single-token decode attention: one new query row against the KV
// cache per (batch, head) — the M=1 GEMV analog of attention. Replaces
// the eager matmul → mask → softmax → matmul chain (and the reference's
// full-sequence recompute, examples/gpt2_inference.cpp:71-122) with two
// tiny kernels: split-KV partials with online softmax, then a combine.
//
// Layout: q [BH, D] bf16; K/V caches [BH, cap, D] bf16 (full fixed-size
// buffers). The live length comes either from a device int64 position
// pointer (len = pos+1; hipGraph-capturable — the grid stays fixed while
// the in-kernel range shrinks) or from a host int. The pointer holds one
// position shared by every row, or one per sequence (ragged batches):
// row bh then reads pos[bh / heads_per_seq].
//
// Partial kernel: grid (BH, SPLITS), 256 threads. Per 256-wide KV tile:
// each thread computes one dot(q, K[i]) (q cached in LDS, K rows read as
// bf16x8 vectors), block-wide online max/sum, P staged through LDS, then
// threads re-map to (d = tid % D, sub = tid / D) and accumulate
// o[d] += p[j] * V[j][d] with consecutive-d coalesced V reads. fp32
// partial o and (m, l) go to a workspace; the combine kernel merges
// splits with the standard flash rescale.

#include "common.h"
#include "kernels.h"

namespace tnn {

template <int D>
__launch_bounds__(256)
__global__ void k_attn_decode(const bf16* __restrict__ q,
                              const bf16* __restrict__ K,
                              const bf16* __restrict__ V,
                              float* __restrict__ po, float* __restrict__ ml,
                              const int64_t* __restrict__ pos_ptr,
                              int pos_div, int len_static, int64_t skv,
                              float scale) {
  constexpr int NSUB = 256 / D;   // sub-accumulators per d column
  constexpr int PER = 256 / NSUB; // tile positions per sub
  const int bh = blockIdx.x;
  const int split = blockIdx.y, NS = gridDim.y;
  // pos_div == 0: one shared position; else rows per sequence (BH / B)
  const int len = pos_ptr ? (int)pos_ptr[pos_div ? bh / pos_div : 0] + 1
                          : len_static;
  const int lo = (int)((int64_t)len * split / NS);
  const int hi = (int)((int64_t)len * (split + 1) / NS);

  const bf16* qr = q + (int64_t)bh * D;
  const bf16* Kb = K + (int64_t)bh * skv;
  const bf16* Vb = V + (int64_t)bh * skv;

  __shared__ float q_lds[D];
  __shared__ float p_lds[256];
  __shared__ float scratch[8];
  __shared__ float bc;  // broadcast slot

  for (int d = threadIdx.x; d < D; d += 256) q_lds[d] = bf2f(qr[d]);
  __syncthreads();

  const int d = threadIdx.x % D;
  const int sub = threadIdx.x / D;
  float m_run = -INFINITY, l_run = 0.0f, o_acc = 0.0f;

  for (int kv0 = lo; kv0 < hi; kv0 += 256) {
    const int i = kv0 + (int)threadIdx.x;
    float sv = -INFINITY;
    if (i < hi) {
      const bf16* krow = &Kb[(int64_t)i * D];
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < D / 8; ++t) {
        bf16x8 kvv = *(const bf16x8*)&krow[t * 8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += q_lds[t * 8 + j] * (float)kvv[j];
      }
      sv = acc * scale;
    }
    float tmax = block_reduce_max(sv, scratch);
    if (threadIdx.x == 0) bc = tmax;
    __syncthreads();
    const float m_new = fmaxf(m_run, bc);
    const float p = (sv == -INFINITY) ? 0.0f : __expf(sv - m_new);
    p_lds[threadIdx.x] = p;
    float tsum = block_reduce_sum(p, scratch);
    if (threadIdx.x == 0) bc = tsum;
    __syncthreads();
    const float alpha = (m_run == -INFINITY) ? 0.0f : __expf(m_run - m_new);
    l_run = l_run * alpha + bc;
    o_acc *= alpha;
#pragma unroll 4
    for (int j = 0; j < PER; ++j) {
      const int t = sub * PER + j;
      if (kv0 + t < hi)
        o_acc += p_lds[t] * bf2f(Vb[(int64_t)(kv0 + t) * D + d]);
    }
    m_run = m_new;
  }

  // fold the NSUB per-d partials (all share m_run/l_run scaling)
  __syncthreads();
  p_lds[threadIdx.x] = o_acc;
  __syncthreads();
  if (sub == 0) {
    float o = 0.0f;
#pragma unroll
    for (int ss = 0; ss < NSUB; ++ss) o += p_lds[ss * D + d];
    po[((int64_t)bh * gridDim.y + split) * D + d] = o;
    if (d == 0) {
      ml[((int64_t)bh * gridDim.y + split) * 2] = m_run;
      ml[((int64_t)bh * gridDim.y + split) * 2 + 1] = l_run;
    }
  }
}

template <int D>
__launch_bounds__(128)
__global__ void k_attn_decode_fin(const float* __restrict__ po,
                                  const float* __restrict__ ml,
                                  bf16* __restrict__ out, int splits) {
  const int bh = blockIdx.x;
  const int d = threadIdx.x;
  if (d >= D) return;
  float m = -INFINITY;
#pragma unroll 4
  for (int s = 0; s < splits; ++s)
    m = fmaxf(m, ml[((int64_t)bh * splits + s) * 2]);
  float l = 0.0f, o = 0.0f;
#pragma unroll 4
  for (int s = 0; s < splits; ++s) {
    const float ms = ml[((int64_t)bh * splits + s) * 2];
    const float ls = ml[((int64_t)bh * splits + s) * 2 + 1];
    if (ls > 0.0f) {
      const float w = __expf(ms - m);
      l += ls * w;
      o += po[((int64_t)bh * splits + s) * D + d] * w;
    }
  }
  out[(int64_t)bh * D + d] = f2bf(l > 0.0f ? o / l : 0.0f);
}

void attn_decode_launch(const void* q, const void* k, const void* v, float* po,
                        float* ml, void* out, const int64_t* pos_ptr,
                        int pos_div, int len_static, int BH, int cap, int D,
                        int splits, float scale, hipStream_t s) {
  dim3 pg(BH, splits);
  const int64_t skv = (int64_t)cap * D;
#define L(DD)                                                                 \
  do {                                                                        \
    hipLaunchKernelGGL(k_attn_decode<DD>, pg, dim3(256), 0, s,                \
                       (const bf16*)q, (const bf16*)k, (const bf16*)v, po,    \
                       ml, pos_ptr, pos_div, len_static, skv, scale);         \
    hipLaunchKernelGGL(k_attn_decode_fin<DD>, dim3(BH), dim3(128), 0, s, po,  \
                       ml, (bf16*)out, splits);                               \
  } while (0)
  if (D == 64) L(64);
  else if (D == 128) L(128);
#undef L
}

// Fused KV append for ragged batches: sequence b's new K and V rows (all
// heads) land at cache position pos[b] in one launch. Caches are dense
// [B,H,cap,D]; the new rows are the strided [B,H,1,D] views of the merged
// QKV projection (element strides sb / sh, unit stride along D).
// Positions are trusted to be < cap (the generation loop clamps them).
template <typename T>
__launch_bounds__(64)
__global__ void k_kv_append(T* __restrict__ kc, T* __restrict__ vc,
                            const T* __restrict__ kn, const T* __restrict__ vn,
                            const int64_t* __restrict__ pos, int H, int cap,
                            int D, int64_t k_sb, int64_t k_sh, int64_t v_sb,
                            int64_t v_sh) {
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int64_t dst = ((int64_t)blockIdx.x * cap + pos[b]) * D;
  const T* ks = kn + b * k_sb + h * k_sh;
  const T* vs = vn + b * v_sb + h * v_sh;
  for (int d = threadIdx.x; d < D; d += 64) {
    kc[dst + d] = ks[d];
    vc[dst + d] = vs[d];
  }
}

void kv_append_launch(DT dt, void* kc, void* vc, const void* kn,
                      const void* vn, const int64_t* pos, int B, int H,
                      int cap, int D, int64_t k_sb, int64_t k_sh, int64_t v_sb,
                      int64_t v_sh, hipStream_t s) {
  if (dt == DT::F32)
    hipLaunchKernelGGL(k_kv_append<float>, dim3(B * H), dim3(64), 0, s,
                       (float*)kc, (float*)vc, (const float*)kn,
                       (const float*)vn, pos, H, cap, D, k_sb, k_sh, v_sb,
                       v_sh);
  else
    hipLaunchKernelGGL(k_kv_append<bf16>, dim3(B * H), dim3(64), 0, s,
                       (bf16*)kc, (bf16*)vc, (const bf16*)kn, (const bf16*)vn,
                       pos, H, cap, D, k_sb, k_sh, v_sb, v_sh);
}

// Multi-row KV append: sequence b's new K/V rows i < n_new[b] (all T when
// n_new is absent) land at cache slot pos[b] + i. Rows that would land at
// >= cap and every row of a negative pos[b] are dropped, so no position
// can make the kernel write outside its sequence's cache. Sources are the
// strided [B,H,T,D] views of the merged projection ({batch, head, row}
// element strides, unit stride along D). One 64-lane block per (row, b*h);
// `vec` (host-checked: 16-byte aligned bases, strides and row size) copies
// 16-byte vectors, else element-wise.
template <typename T>
__launch_bounds__(64)
__global__ void k_kv_append_n(T* __restrict__ kc, T* __restrict__ vc,
                              const T* __restrict__ kn,
                              const T* __restrict__ vn,
                              const int64_t* __restrict__ pos,
                              const int64_t* __restrict__ n_new, int Tn, int H,
                              int cap, int D, int64_t k_sb, int64_t k_sh,
                              int64_t k_sr, int64_t v_sb, int64_t v_sh,
                              int64_t v_sr, bool vec) {
  const int i = blockIdx.x;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int64_t p = pos[b];
  const int64_t n = n_new ? n_new[b] : (int64_t)Tn;
  if (p < 0 || i >= n || p + i >= cap) return;
  const int64_t dst = ((int64_t)blockIdx.y * cap + p + i) * D;
  const T* ks = kn + b * k_sb + h * k_sh + i * k_sr;
  const T* vs = vn + b * v_sb + h * v_sh + i * v_sr;
  if (vec) {
    constexpr int V = 16 / (int)sizeof(T);
    for (int d = threadIdx.x * V; d < D; d += 64 * V) {
      *(uint4*)&kc[dst + d] = *(const uint4*)&ks[d];
      *(uint4*)&vc[dst + d] = *(const uint4*)&vs[d];
    }
  } else {
    for (int d = threadIdx.x; d < D; d += 64) {
      kc[dst + d] = ks[d];
      vc[dst + d] = vs[d];
    }
  }
}

void kv_append_n_launch(DT dt, void* kc, void* vc, const void* kn,
                        const void* vn, const int64_t* pos,
                        const int64_t* n_new, int B, int H, int T, int cap,
                        int D, const int64_t* k_str, const int64_t* v_str,
                        bool vec, hipStream_t s) {
#define L(TT)                                                                 \
  hipLaunchKernelGGL(k_kv_append_n<TT>, dim3(T, B * H), dim3(64), 0, s,       \
                     (TT*)kc, (TT*)vc, (const TT*)kn, (const TT*)vn, pos,     \
                     n_new, T, H, cap, D, k_str[0], k_str[1], k_str[2],       \
                     v_str[0], v_str[1], v_str[2], vec)
  if (dt == DT::F32) L(float);
  else L(bf16);
#undef L
}

}  // namespace tnn
