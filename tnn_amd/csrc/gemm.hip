// MFMA GEMM kernels: NN (fused bias+activation epilogue), NT (dgrad),
// TN (wgrad: deterministic split-M fp32 slabs + casting reduce), plus
// M=1 GEMV forms for the decode path.
// Replaces the reference's cublasGemmEx / cuDNN-frontend matmul call sites
// (src/math/cuda/gemm.cu:64, src/math/cuda/cudnn_gemm.cu:285,
// src/nn/layers_impl/cuda/dense_ops.cu:17-117).

#include <stdexcept>
#include "common.h"
#include "kernels.h"
#include "tile_gemm.h"

namespace tnn {

using namespace tile;

// ---------------------------------------------------------------------------
// pieces shared by every route
// ---------------------------------------------------------------------------

// The one fused epilogue: act(v + bias[col]) + resid[row, col], all in
// fp32 — the order of the eager path in ops/functional.py::linear. Null
// bias / resid and ACT_LINEAR skip their step.
template <typename T>
struct Epilogue {
  const T* bias;
  const T* resid;
  int ldc;  // row stride of resid
  int act;
  // resid addressed by flat element index (for callers that already
  // hold row * ldc + col)
  DEV float at(float v, int col, int64_t idx) const {
    if (bias) v += VecIO<T>::to_f32(bias[col]);
    if (act != ACT_LINEAR) v = act_apply(v, act);
    if (resid) v += VecIO<T>::to_f32(resid[idx]);
    return v;
  }
  DEV float operator()(float v, int row, int col) const {
    return at(v, col, (int64_t)row * ldc + col);
  }
};

// Stage ROWS k-contiguous rows src[row0 + r][k0 .. k0 + BK) (row stride K)
// as the swizzled LDS image dst[r][k]; rows >= nrows and k >= K are zero.
template <typename T, int ROWS>
DEV void stage_rows(T* dst, const T* __restrict__ src, int row0, int nrows,
                    int k0, int K) {
  constexpr int V = 16 / sizeof(T);
#pragma unroll
  for (int c = threadIdx.x; c < ROWS * (BK / V); c += THREADS) {
    int row = c / (BK / V);
    int kk = (c % (BK / V)) * V;
    int g = row0 + row;
    Pack16<T> v = {};
    if (g < nrows) v = load16_guarded(&src[(int64_t)g * K], k0 + kk, K);
    *(Pack16<T>*)&dst[lds_off<T>(row, kk)] = v;
  }
}

// The same image by LDS-DMA (K % V == 0, 16B-aligned src): rows >= nrows
// and k >= k_hi read the zero page.
template <typename T, int ROWS>
DEV void glds_stage_rows(T* dst, const WaveCoord& wc,
                         const T* __restrict__ src,
                         const T* __restrict__ zero16, int row0, int nrows,
                         int K, int k0, int k_hi) {
  glds_stage<T, ROWS>(dst, wc, [&](int rl, int kk) -> const T* {
    int g = row0 + rl, gk = k0 + kk;
    if (g >= nrows || gk >= k_hi) return zero16;
    return &src[(int64_t)g * K + gk];
  });
}

// Stage src[k0 + k][c0 .. c0 + COLS) (row-major, ld columns, rows < k_end)
// transposed, as the image dst[c][k]: column-contiguous vector loads,
// element scatter into LDS.
template <typename T, int COLS>
DEV void stage_transposed(T* dst, const T* src, int ld, int k0,
                          int k_end, int c0) {
  constexpr int V = 16 / sizeof(T);
#pragma unroll 1  // full unroll quadruples live address state (spills)
  for (int c = threadIdx.x; c < BK * (COLS / V); c += THREADS) {
    int kk = c / (COLS / V);
    int cc = (c % (COLS / V)) * V;
    int gk = k0 + kk;
    Pack16<T> v = {};
    if (gk < k_end) v = load16_guarded(&src[(int64_t)gk * ld], c0 + cc, ld);
#pragma unroll
    for (int j = 0; j < V; ++j)
      dst[lds_off<T>(cc + j, kk)] = v.e[j];
  }
}

// cast store of one 16x16-core block tile through the fused epilogue
template <typename T>
DEV void epilogue_store(const WaveCoord& wc, f32x4 acc[FM][FN], T* C, int m0,
                        int n0, int M, int N, const Epilogue<T>& ep) {
  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < N)
      C[(int64_t)row * N + col] = VecIO<T>::from_f32(ep(v, row, col));
  });
}

// fp32 slab store: block z owns slab z of the [gridDim.z][rows][cols]
// workspace (the output itself when unsplit); a separate reduce pass sums
// the slabs — deterministic, no atomic contention
DEV void slab_store(const WaveCoord& wc, f32x4 acc[FM][FN], float* ws,
                    int row0, int col0, int rows, int cols) {
  float* out = ws + (int64_t)blockIdx.z * rows * cols;
  epilogue_visit(wc, acc, row0, col0, [&](int row, int col, float v) {
    if (row < rows && col < cols) out[(int64_t)row * cols + col] = v;
  });
}

// this block's BK-aligned slice [k_lo, k_hi) of a K reduction split over
// grid.z (the whole of K when gridDim.z == 1)
DEV void ksplit_range(int K, int& k_lo, int& k_hi) {
  const int Z = gridDim.z;
  k_lo = (int)(((int64_t)K * blockIdx.z / Z) / BK * BK);
  k_hi = blockIdx.z + 1 == Z
             ? K
             : (int)(((int64_t)K * (blockIdx.z + 1) / Z) / BK * BK);
}

// Double-buffered global_load_lds main loop over k in [k_lo, k_hi) for NT
// operands (A[M,K] and B[N,K] rows are both k-contiguous, so the next
// chunk's LDS-DMAs overlap the current chunk's MFMAs). Rows past M / N
// and k past k_hi read the zero page. compute(As, Bs) consumes one
// staged [BM][BK] x [BN][BK] chunk.
template <typename T, typename Compute>
DEV void nt_db_mainloop(const T* __restrict__ A, const T* __restrict__ B,
                        const T* __restrict__ zero16, T (&As)[2][BM * BK],
                        T (&Bs)[2][BN * BK], const WaveCoord& wc, int m0,
                        int n0, int M, int N, int K, int k_lo, int k_hi,
                        Compute&& compute) {
  auto stage = [&](int kk0, int which) {
    glds_stage_rows<T, BM>(As[which], wc, A, zero16, m0, M, K, kk0, k_hi);
    glds_stage_rows<T, BN>(Bs[which], wc, B, zero16, n0, N, K, kk0, k_hi);
  };
  constexpr int NPER = glds_count<T, BM>() + glds_count<T, BN>();

  const int nch = (k_hi - k_lo + BK - 1) / BK;
  stage(k_lo, 0);
  for (int t = 0; t < nch; ++t) {
    const int cur = t & 1;
    if (t + 1 < nch) {
      stage(k_lo + (t + 1) * BK, cur ^ 1);
      wait_vmcnt<NPER>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    compute(As[cur], Bs[cur]);
    __builtin_amdgcn_s_barrier();
  }
}

// ---------------------------------------------------------------------------
// NN / NT kernel: C[M,N] = act(A[M,K] @ B + bias) + resid
//   TRANS_B = false: B is [K, N] row-major (staged transposed into LDS)
//   TRANS_B = true:  B is [N, K] row-major (staged directly; C = A @ B^T)
// ---------------------------------------------------------------------------

template <typename T, bool TRANS_B, bool GLDS>
__launch_bounds__(THREADS)
__global__ void k_gemm(const T* __restrict__ A, const T* __restrict__ B,
                       const T* __restrict__ bias, T* __restrict__ C,
                       const T* __restrict__ zero16,
                       const T* __restrict__ resid, int M, int N, int K,
                       int act_kind) {
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];

  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  for (int k0 = 0; k0 < K; k0 += BK) {
    // A[M,K] and (TRANS_B) B[N,K] rows are already the image rows. GLDS:
    // K % V == 0 and 16B-aligned A (and B, when TRANS_B) guaranteed by
    // the launcher.
    if constexpr (GLDS)
      glds_stage_rows<T, BM>(As, wc, A, zero16, m0, M, K, k0, K);
    else
      stage_rows<T, BM>(As, A, m0, M, k0, K);
    if constexpr (TRANS_B && GLDS)
      glds_stage_rows<T, BN>(Bs, wc, B, zero16, n0, N, K, k0, K);
    else if constexpr (TRANS_B)
      stage_rows<T, BN>(Bs, B, n0, N, k0, K);
    else  // B[K,N]: n-contiguous loads, scatter-transposed into Bs[n][k]
      stage_transposed<T, BN>(Bs, B, N, k0, K, n0);
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }

  epilogue_store(wc, acc, C, m0, n0, M, N, {bias, resid, N, act_kind});
}

// ---------------------------------------------------------------------------
// TN kernel: C[K,N] = A[M,K]^T @ B[M,N] into per-slice fp32 slabs.
// Grid.z slices the M reduction (split-K in the GEMM sense) so small-output
// wgrads still fill 256 CUs (SURVEY §7 hard part 1).
// ---------------------------------------------------------------------------

template <typename T>
__launch_bounds__(THREADS, 3)  // cap VGPRs: unconstrained allocation hit 221-256 VGPR = 1-2 waves/SIMD
__global__ void k_gemm_tn(const T* __restrict__ A, const T* __restrict__ B,
                          float* __restrict__ C, int M, int N, int K) {
  __shared__ alignas(16) T As[BM * BK];  // rows = K-dim, k = m-chunk
  __shared__ alignas(16) T Bs[BN * BK];

  const int r0 = blockIdx.x * BM;  // output row = A column
  const int n0 = blockIdx.y * BN;
  // 32-bit m index: int64 div/mod in the staging loop costs ~100 VALU
  // cycles per chunk (measured: wgrad at 1/4 the MFMA residency of fwd)
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  for (int k0 = m_begin; k0 < m_end; k0 += BK) {
    stage_transposed<T, BM>(As, A, K, k0, m_end, r0);  // A[m][r] -> As[r][m]
    stage_transposed<T, BN>(Bs, B, N, k0, m_end, n0);  // B[m][n] -> Bs[n][m]
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }

  slab_store(wc, acc, C, r0, n0, K, N);
}

// double-buffered pure-glds NT gemm (see k_conv_fwd_db and
// nt_db_mainloop). Dispatched for K <= 3072 (2x LDS buffers cap
// occupancy at 3 blocks/CU; long k-loops prefer the 6-block single-buffer
// kernel).
template <typename T>
__launch_bounds__(THREADS)
__global__ void k_gemm_nt_db(const T* __restrict__ A, const T* __restrict__ B,
                             const T* __restrict__ bias, T* __restrict__ C,
                             const T* __restrict__ zero16,
                             const T* __restrict__ resid, int M, int N, int K,
                             int act_kind) {
  __shared__ alignas(16) T As[2][BM * BK];
  __shared__ alignas(16) T Bs[2][BN * BK];
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  nt_db_mainloop(A, B, zero16, As, Bs, wc, m0, n0, M, N, K, 0, K,
                 [&](const T* as, const T* bs) {
                   mfma_compute_tile(as, bs, wc, acc);
                 });

  epilogue_store(wc, acc, C, m0, n0, M, N, {bias, resid, N, act_kind});
}

// M=1 NT matvec (decode-path linears): one wave per output row, 16B loads
// over K, cross-lane reduce. The MFMA tile kernel wastes 127/128 of its
// A-tile rows at M=1 and is ~30x slower on gpt2 decode shapes.
template <typename T>
__launch_bounds__(256)
__global__ void k_gemv_nt(const T* __restrict__ x, const T* __restrict__ B,
                          const T* __restrict__ bias,
                          const T* __restrict__ resid, T* __restrict__ y,
                          int N, int K, int act_kind) {
  constexpr int V = 16 / sizeof(T);
  using VecT = Pack16<T>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  const T* row = &B[(int64_t)n * K];
  float acc = 0.0f;
  if ((K % V) == 0 && aligned16(row) && aligned16(x)) {
    for (int k = lane * V; k < K; k += 64 * V) {
      VecT vb = *(const VecT*)&row[k];
      VecT vx = *(const VecT*)&x[k];
#pragma unroll
      for (int j = 0; j < V; ++j)
        acc += VecIO<T>::to_f32(vx.e[j]) * VecIO<T>::to_f32(vb.e[j]);
    }
  } else {
    for (int k = lane; k < K; k += 64)
      acc += VecIO<T>::to_f32(x[k]) * VecIO<T>::to_f32(row[k]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_xor(acc, off, 64);
  if (lane == 0)
    y[n] = VecIO<T>::from_f32(
        Epilogue<T>{bias, resid, N, act_kind}(acc, 0, n));
}

// K-split NT gemm for huge-K underfilled shapes (the GPT-2 vocab-head
// dgrad: dx[4096,768] = dy[4096,50264] @ W^T — 384 blocks and a 785-
// chunk k-loop on the plain kernel, 313 TF). grid.z slices K; each
// slice writes an fp32 slab, the split-K reduce (shared with wgrad)
// sums and casts. Same double-buffered main loop as k_gemm_nt_db.
template <typename T>
__launch_bounds__(THREADS)
__global__ void k_gemm_nt_z(const T* __restrict__ A, const T* __restrict__ B,
                            float* __restrict__ Cws,
                            const T* __restrict__ zero16, int M, int N,
                            int K) {
  __shared__ alignas(16) T As[2][BM * BK];
  __shared__ alignas(16) T Bs[2][BN * BK];
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  int k_lo, k_hi;
  ksplit_range(K, k_lo, k_hi);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  nt_db_mainloop(A, B, zero16, As, Bs, wc, m0, n0, M, N, K, k_lo, k_hi,
                 [&](const T* as, const T* bs) {
                   mfma_compute_tile(as, bs, wc, acc);
                 });

  slab_store(wc, acc, Cws, m0, n0, M, N);
}

// ---------------------------------------------------------------------------
// 32x32x16-MFMA NT GEMM (bf16): the 16x16x32 tile core needs 3-4 waves
// per SIMD to cover its ~17 cyc/SIMD single-wave issue floor, but
// v_mfma_f32_32x32x16_bf16 sustains PEAK issue at ONE wave/SIMD
// (MI355X_MICROARCH.md cycle table) and touches half the LDS bytes per
// FLOP (A/B reuse 32 wide, not 16). Same 128x64 block tile and BK=64 as
// the 16x16 core (4 M-stacked waves of 32x64, two 32x32 fragments each),
// the shared double-buffered glds main loop, optional K-split over
// blockIdx.z into fp32 slabs (finalized by k_splitk_fin_ep with the
// bias/act/residual epilogue).
#ifndef GEMM_REMAP_GM
#define GEMM_REMAP_GM 8
#endif

// C/D map for 32x32x16 (guide: col = lane&31, row = (reg&3) + 8*(reg>>2)
// + 4*(lane>>5), reg in [0,16))
template <typename T>
__launch_bounds__(256)
__global__ void k_gemm_nt32(const T* __restrict__ A, const T* __restrict__ B,
                            const T* __restrict__ bias, T* __restrict__ C,
                            float* __restrict__ Cws,
                            const T* __restrict__ zero16,
                            const T* __restrict__ resid, int M, int N, int K,
                            int act_kind) {
  __shared__ alignas(16) T As[2][BM * BK];
  __shared__ alignas(16) T Bs[2][BN * BK];
  int tm, tn;
  // grouped ordering pays only when the re-read streams exceed the
  // 256 MiB L3 (vocab-head-sized operands measured +9%; L3-resident
  // shapes were flat-to-negative)
  if ((int64_t)M * N + (int64_t)N * K > (int64_t)48 * 1024 * 1024)
    tile_remap<GEMM_REMAP_GM>(tm, tn);
  else {
    tm = blockIdx.x;
    tn = blockIdx.y;
  }
  const int m0 = tm * BM;
  const int n0 = tn * BN;
  const int Z = gridDim.z;
  int k_lo, k_hi;
  ksplit_range(K, k_lo, k_hi);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wrow0 = wid * 32;   // 4 M-stacked waves: 32 rows x 64 cols each
  const WaveCoord wc;  // only for glds_stage lane bookkeeping

  f32x16 acc[2] = {};

  // a-frag: lane supplies row (lane&31), k (lane>>5)*8..+8
  const int ar = lane & 31;
  const int kh = (lane >> 5) * 8;
  nt_db_mainloop(A, B, zero16, As, Bs, wc, m0, n0, M, N, K, k_lo, k_hi,
                 [&](const T* as, const T* bs) {
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const int kb = ks * 16 + kh;
      bf16x8 a, b[2];
      a = *(const bf16x8*)&as[lds_off<T>(wrow0 + ar, kb)];
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
        b[fn] = *(const bf16x8*)&bs[lds_off<T>(fn * 32 + ar, kb)];
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
        acc[fn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a, b[fn], acc[fn], 0, 0, 0);
    }
  });

  const Epilogue<T> ep{bias, resid, N, act_kind};
  const int cc = lane & 31;
  const int r4 = (lane >> 5) * 4;
#pragma unroll
  for (int fn = 0; fn < 2; ++fn)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = m0 + wrow0 + (reg & 3) + 8 * (reg >> 2) + r4;
      const int col = n0 + fn * 32 + cc;
      if (row >= M || col >= N) continue;
      const float vv = acc[fn][reg];
      if (Z > 1)
        Cws[(int64_t)blockIdx.z * M * N + (int64_t)row * N + col] = vv;
      else
        C[(int64_t)row * N + col] = VecIO<T>::from_f32(ep(vv, row, col));
    }
}

// split-K for moderately underfilled FORWARD NT shapes (e.g. the
// transformer's [B*S, 768] projections: 384 blocks on 256 CUs ran at
// ~170 TF while full-grid launches of the same kernel reach ~2.3x
// that): fill to ~3 blocks/CU, epilogue moves into the fused finalize.
int gemm_nt_fsplits(DT dt, int M, int N, int K) {
  const int base = ceil_div(M, BM) * ceil_div(N, BN);
  if (base >= 768 || K < 4 * BK) return 1;
  if (K % vec_elems(dt) != 0) return 1;
  return std::min(ceil_div(768, base), K / (2 * BK));
}

// fused split-K finalize: fold the Z fp32 slabs, then the same Epilogue
// the direct kernels apply (relocated here for the z-split routes), cast
// to T
template <typename T>
__launch_bounds__(256)
__global__ void k_splitk_fin_ep(const float4* __restrict__ ws,
                                const T* __restrict__ bias,
                                const T* __restrict__ resid,
                                T* __restrict__ out, int z, int N,
                                int64_t n4, int act_kind) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  struct alignas(4 * sizeof(T)) T4 { T e[4]; };
  const Epilogue<T> ep{bias, resid, N, act_kind};
  for (; i < n4; i += stride) {
    float4 a{0.0f, 0.0f, 0.0f, 0.0f};
    for (int sl = 0; sl < z; ++sl) {
      float4 v = ws[(int64_t)sl * n4 + i];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    float r[4] = {a.x, a.y, a.z, a.w};
    const int col0 = (int)((i * 4) % N);
    T4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o.e[j] = VecIO<T>::from_f32(ep.at(r[j], col0 + j, i * 4 + j));
    ((T4*)out)[i] = o;
  }
}

// finalize launch shared by both split-K forward routes (N % 4 == 0
// enforced by the callers)
template <typename T>
static void splitk_fin_ep_launch(const float* ws, const void* bias,
                                 const void* resid, void* c, int z, int M,
                                 int N, int act_kind, hipStream_t s) {
  const int64_t n4 = (int64_t)M * N / 4;
  int blocks = (int)std::min<int64_t>((n4 + 255) / 256, (int64_t)2048);
  hipLaunchKernelGGL(k_splitk_fin_ep<T>, dim3(blocks), dim3(256), 0, s,
                     (const float4*)ws, (const T*)bias, (const T*)resid,
                     (T*)c, z, N, n4, act_kind);
}

template <typename T>
static void gemm_nt_z_kernel_launch(const void* a, const void* b, float* ws,
                                    int z, const void* zero16, int M, int N,
                                    int K, hipStream_t s) {
  dim3 grid(ceil_div(M, BM), ceil_div(N, BN), z);
  hipLaunchKernelGGL(k_gemm_nt_z<T>, grid, dim3(THREADS), 0, s, (const T*)a,
                     (const T*)b, ws, (const T*)zero16, M, N, K);
}

void gemm_nt_zf_launch(DT dt, const void* a, const void* b, float* ws,
                       const void* bias, const void* resid, void* c, int z,
                       const void* zero16, int M, int N, int K, int act_kind,
                       hipStream_t s) {
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    gemm_nt_z_kernel_launch<T>(a, b, ws, z, zero16, M, N, K, s);
    splitk_fin_ep_launch<T>(ws, bias, resid, c, z, M, N, act_kind, s);
  });
}

// K-splits for the 32-wide NT kernel: fill to ~2 blocks/CU (its LDS
// footprint caps residency at 2)
int gemm_nt32_zsplits(int M, int N, int K) {
  const int base = ceil_div(M, BM) * ceil_div(N, BN);
  if (base >= 512 || K < 4 * BK) return 1;
  if (K % 8 != 0) return 1;
  return std::min(ceil_div(512, base), K / (2 * BK));
}

void gemm_nt32_launch(const void* a, const void* b, float* ws,
                      const void* bias, const void* resid, void* c, int z,
                      const void* zero16, int M, int N, int K, int act_kind,
                      hipStream_t s) {
  dim3 grid(ceil_div(M, BM), ceil_div(N, BN), z);
  hipLaunchKernelGGL(k_gemm_nt32<bf16>, grid, dim3(256), 0, s, (const bf16*)a,
                     (const bf16*)b, (const bf16*)bias, (bf16*)c, ws,
                     (const bf16*)zero16, (const bf16*)resid, M, N, K,
                     act_kind);
  if (z > 1)
    splitk_fin_ep_launch<bf16>(ws, bias, resid, c, z, M, N, act_kind, s);
}

int gemm_nt_zsplits(DT dt, int M, int N, int K) {
  const int base = ceil_div(M, BM) * ceil_div(N, BN);
  if (base >= 768 || K < 4 * BK) return 1;
  if (K % vec_elems(dt) != 0) return 1;
  return std::min(ceil_div(K, 4 * BK), ceil_div(1024, base));
}

void gemm_nt_z_launch(DT dt, const void* a, const void* b, float* ws,
                      void* c_out, DT out_dt, int z, const void* zero16,
                      int M, int N, int K, hipStream_t s) {
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    gemm_nt_z_kernel_launch<T>(a, b, ws, z, zero16, M, N, K, s);
  });
  splitk_reduce_launch(ws, c_out, out_dt, z, (int64_t)M * N, s);
}

// Single-launch M=1 NN matvec: out[N] = x[K] @ B[K,N], x cached in LDS,
// bias/activation/residual fused into the epilogue. The two-kernel
// K-split form below measured 23us per decode linear (its finalize is a
// 48-deep serial slab reduce on 3 blocks); this is one latency-bound
// pass (~2-3us). Blocks own 64 n-columns; the 4 thread-rows split K and
// fold through LDS. K <= GEMV1_MAX_K (x LDS cache); larger K falls back.
template <typename T>
__launch_bounds__(256)
__global__ void k_gemv_nn1(const T* __restrict__ x, const T* __restrict__ B,
                           const T* __restrict__ bias,
                           const T* __restrict__ res, T* __restrict__ y,
                           float* __restrict__ part,
                           const float* __restrict__ ln_g,
                           const float* __restrict__ ln_b, float ln_eps,
                           int N, int K, int act_kind) {
  __shared__ float xs[GEMV1_MAX_K];
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63;
  const int ks = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + c;
  // this block's K slice (grid.y = nsplit; 4-aligned so the thread-row
  // interleave stays uniform)
  const int nsplit = gridDim.y;
  const int k_lo = (int)(((int64_t)K * blockIdx.y / nsplit) & ~3LL);
  const int k_hi = blockIdx.y + 1 == nsplit
                       ? K
                       : (int)(((int64_t)K * (blockIdx.y + 1) / nsplit) & ~3LL);
  if (ln_g) {
    // fused LayerNorm on the x vector (decode: saves the separate ln
    // kernel + its memory round trip; every split block recomputes the
    // row stats — trivial next to the per-kernel floor)
    for (int k = threadIdx.x; k < K; k += 256)
      xs[k] = VecIO<T>::to_f32(x[k]);
    __syncthreads();
    float sm = 0.0f;
    for (int k = threadIdx.x; k < K; k += 256) sm += xs[k];
    sm = block_reduce_sum(sm, red[0]);
    __shared__ float bmean;
    if (threadIdx.x == 0) bmean = sm / (float)K;
    __syncthreads();
    // centred variance from the LDS copy (matches ln_fwd; the raw
    // E[x^2] - mean^2 form cancels in fp32 once |mean| >> std). The same
    // pass sums x - mu: that residual dm is what fp32 rounding cut off the
    // mean (up to ulp(mean)/2, which is 1e-5 of a std at mean/std = 256).
    // x - mu is exact there, so (x - mu) - dm centres on the true mean;
    // dm^2 <= 2^-48 mean^2 is left out of the variance.
    const float mu = bmean;
    float sq = 0.0f, sd = 0.0f;
    for (int k = threadIdx.x; k < K; k += 256) {
      const float d = xs[k] - mu;
      sq += d * d;
      sd += d;
    }
    sq = block_reduce_sum(sq, red[0]);
    sd = block_reduce_sum(sd, red[1]);
    __shared__ float binv, bdm;
    if (threadIdx.x == 0) {
      binv = rsqrtf(sq / (float)K + ln_eps);
      bdm = sd / (float)K;
    }
    __syncthreads();
    const float is = binv, dm = bdm;
    for (int k = k_lo + (int)threadIdx.x; k < k_hi; k += 256)
      xs[k] = ((xs[k] - mu) - dm) * is * ln_g[k] + ln_b[k];
    __syncthreads();
  } else {
    for (int k = k_lo + (int)threadIdx.x; k < k_hi; k += 256)
      xs[k] = VecIO<T>::to_f32(x[k]);
    __syncthreads();
  }
  float acc = 0.0f;
  if (n < N) {
    int k = k_lo + ks;
    // batched 8-deep loads, then the FMAs: keeps 8 loads in flight per
    // thread instead of a serialized load-fma chain
    for (; k + 32 <= k_hi; k += 32) {
      float bv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        bv[u] = VecIO<T>::to_f32(B[(int64_t)(k + 4 * u) * N + n]);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += xs[k + 4 * u] * bv[u];
    }
    for (; k < k_hi; k += 4)
      acc += xs[k] * VecIO<T>::to_f32(B[(int64_t)k * N + n]);
  }
  red[ks][c] = acc;
  __syncthreads();
  if (ks == 0 && n < N) {
    float a = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    if (part) {
      part[(int64_t)blockIdx.y * N + n] = a;
      return;
    }
    y[n] = VecIO<T>::from_f32(Epilogue<T>{bias, res, N, act_kind}(a, 0, n));
  }
}

// parallel finalize over n: sum <= 16 fp32 partial rows + fused epilogue
template <typename T>
__launch_bounds__(256)
__global__ void k_gemv_fin2(const float* __restrict__ part,
                            const T* __restrict__ bias,
                            const T* __restrict__ res, T* __restrict__ y,
                            int N, int nsplit, int act_kind) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  int s = 0;
  for (; s + 4 <= nsplit; s += 4) {
    a0 += part[(int64_t)s * N + n];
    a1 += part[(int64_t)(s + 1) * N + n];
    a2 += part[(int64_t)(s + 2) * N + n];
    a3 += part[(int64_t)(s + 3) * N + n];
  }
  for (; s < nsplit; ++s) a0 += part[(int64_t)s * N + n];
  const float a = (a0 + a1) + (a2 + a3);
  y[n] = VecIO<T>::from_f32(Epilogue<T>{bias, res, N, act_kind}(a, 0, n));
}

int gemv_nn1_nsplit(int N, int K) {
  // fill the chip: blocks = (N/64) * nsplit ~ 256; keep slices >= 64 rows
  int ncb = ceil_div(N, 64);
  int ns = std::max(1, std::min(16, 256 / ncb));
  ns = std::min(ns, std::max(1, K / 64));
  return ns;
}

void gemv_nn1_launch(DT dt, const void* x, const void* b, const void* bias,
                     const void* res, void* y, float* part, int nsplit,
                     const float* ln_g, const float* ln_b, float ln_eps, int N,
                     int K, int act_kind, hipStream_t s) {
  dim3 g(ceil_div(N, 64), nsplit);
  dim3 fg(ceil_div(N, 256));
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_gemv_nn1<T>, g, dim3(256), 0, s, (const T*)x,
                       (const T*)b, (const T*)bias, (const T*)res, (T*)y,
                       nsplit > 1 ? part : nullptr, ln_g, ln_b, ln_eps, N, K,
                       act_kind);
    if (nsplit > 1)
      hipLaunchKernelGGL(k_gemv_fin2<T>, fg, dim3(256), 0, s, part,
                         (const T*)bias, (const T*)res, (T*)y, N, nsplit,
                         act_kind);
  });
}

// ---------------------------------------------------------------------------
// Skinny NN GEMM for batched decode, 2 <= M <= 16:
//   y[M,N] = act(LN?(x)[M,K] @ B[K,N] + bias) + resid
// Decode is weight-bandwidth-bound, so every B element is fetched once and
// applied to all M rows: B streams straight into VGPRs (8-deep batched
// loads, two columns per lane, no LDS round trip) while the block's
// K-chunk of the M x rows sits in LDS as fp32 [k][MT] and is read back as
// wave-uniform broadcasts. Blocks own 128 columns x one K slice (grid.y);
// the block's 4 waves interleave the slice's k rows and fold through LDS.
// With grid.y > 1 the block writes fp32 partials [split][M][N] and
// k_skinny_fin folds them in a fixed order (deterministic, no atomics).
// Any N and K: rows whose 2-column pairs cannot be loaded as one aligned
// word (odd N) take the element-wise column mapping instead.
// ---------------------------------------------------------------------------
constexpr int SK_COLS = 128;  // columns per block
constexpr int SK_KC = 512;    // k rows of x staged per LDS chunk
constexpr int SK_U = 8;       // B loads in flight per lane
constexpr int SK_LN_RC = 16;  // fused-LN row elements a lane keeps (K <= 1024)

// One lane's two B elements of row `off / N`. c0 / c1 are already
// clamped into the row by the caller, so the loads are unconditional: a
// load under a lane-dependent branch is waited for inside that branch,
// which serialises the SK_U loads a batch is meant to keep in flight.
template <typename T, bool VEC>
DEV void sk_load(const T* __restrict__ B, int64_t off, int c0, int c1,
                 float& w0, float& w1) {
  if constexpr (VEC) {  // c0 even, N even: one aligned pair
    struct alignas(2 * sizeof(T)) P2 { T e[2]; };
    const P2 p = *(const P2*)&B[off + c0];
    w0 = VecIO<T>::to_f32(p.e[0]);
    w1 = VecIO<T>::to_f32(p.e[1]);
  } else {
    w0 = VecIO<T>::to_f32(B[off + c0]);
    w1 = VecIO<T>::to_f32(B[off + c1]);
  }
}

// one staged chunk: this wave's rows kk = wave, wave + 4, ... < kc_n
template <typename T, int MT, bool VEC>
DEV void sk_chunk(const T* __restrict__ B, const float* xs, int N, int kc0,
                  int kc_n, int wave, int c0, int c1, float (&acc)[MT][2]) {
  // columns past N read the row's last pair / element instead; their
  // accumulators are never stored
  c0 = min(c0, VEC ? N - 2 : N - 1);
  c1 = min(c1, N - 1);
  int kk = wave;
  for (; kk + 4 * (SK_U - 1) < kc_n; kk += 4 * SK_U) {
    float w0[SK_U], w1[SK_U];
#pragma unroll
    for (int u = 0; u < SK_U; ++u)
      sk_load<T, VEC>(B, (int64_t)(kc0 + kk + 4 * u) * N, c0, c1, w0[u],
                      w1[u]);
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const float* xr = &xs[(kk + 4 * u) * MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[m][0] += xr[m] * w0[u];
        acc[m][1] += xr[m] * w1[u];
      }
    }
  }
  for (; kk < kc_n; kk += 4) {
    float w0, w1;
    sk_load<T, VEC>(B, (int64_t)(kc0 + kk) * N, c0, c1, w0, w1);
    const float* xr = &xs[kk * MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      acc[m][0] += xr[m] * w0;
      acc[m][1] += xr[m] * w1;
    }
  }
}

template <typename T, int MT>
__launch_bounds__(256)
__global__ void k_gemm_skinny(const T* __restrict__ x, const T* __restrict__ B,
                              const T* __restrict__ bias,
                              const T* __restrict__ res, T* __restrict__ y,
                              float* __restrict__ part,
                              const float* __restrict__ ln_g,
                              const float* __restrict__ ln_b, float ln_eps,
                              int M, int N, int K, int act_kind, int vec) {
  constexpr int XS = SK_KC * MT;
  constexpr int RED = 3 * MT * SK_COLS;
  __shared__ alignas(16) float buf[XS > RED ? XS : RED];
  __shared__ float mu_s[MT], dm_s[MT], is_s[MT];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * SK_COLS;
  // accumulator j of this lane: adjacent columns (one aligned pair load)
  // or lane-strided columns (element loads, wave-contiguous per j)
  const int c0 = vec ? n0 + 2 * lane : n0 + lane;
  const int c1 = vec ? c0 + 1 : c0 + 64;
  const int nsplit = gridDim.y;
  const int k_lo = (int)((int64_t)K * blockIdx.y / nsplit);
  const int k_hi = (int)((int64_t)K * (blockIdx.y + 1) / nsplit);

  if (ln_g) {
    // per-row LayerNorm statistics over the full row (recomputed by every
    // block, as in k_gemv_nn1): one wave per row
    for (int m = wave; m < M; m += 4) {
      // two passes, centred on the mean. Rows of up to 64 * SK_LN_RC
      // elements stay in registers between them (unconditional clamped
      // loads, see sk_load); longer rows are read again from cache.
      const T* xr = x + (int64_t)m * K;
      const bool cached = K <= 64 * SK_LN_RC;
      float xv[SK_LN_RC];
      float sm = 0.0f;
      if (cached) {
#pragma unroll
        for (int i = 0; i < SK_LN_RC; ++i) {
          const int k = lane + 64 * i;
          const float v = VecIO<T>::to_f32(xr[min(k, K - 1)]);
          xv[i] = k < K ? v : 0.0f;
          sm += xv[i];
        }
      } else {
        for (int k = lane; k < K; k += 64) sm += VecIO<T>::to_f32(xr[k]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off, 64);
      // dm is the mean's fp32 rounding residual, as in k_gemv_nn1
      const float mean = sm / (float)K;
      float sq = 0.0f, sd = 0.0f;
      if (cached) {
#pragma unroll
        for (int i = 0; i < SK_LN_RC; ++i) {
          const float d = lane + 64 * i < K ? xv[i] - mean : 0.0f;
          sq += d * d;
          sd += d;
        }
      } else {
        for (int k = lane; k < K; k += 64) {
          const float d = VecIO<T>::to_f32(xr[k]) - mean;
          sq += d * d;
          sd += d;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sq += __shfl_xor(sq, off, 64);
        sd += __shfl_xor(sd, off, 64);
      }
      if (lane == 0) {
        mu_s[m] = mean;
        dm_s[m] = sd / (float)K;
        is_s[m] = rsqrtf(sq / (float)K + ln_eps);
      }
    }
    __syncthreads();
  }

  float acc[MT][2] = {};
  for (int kc0 = k_lo; kc0 < k_hi; kc0 += SK_KC) {
    const int kc_n = min(SK_KC, k_hi - kc0);
    // stage x[0..MT)[kc0 .. kc0 + kc_n) as fp32 [k][MT]; rows >= M are zero
    for (int i = threadIdx.x; i < kc_n * MT; i += 256) {
      const int m = i / kc_n, kk = i - m * kc_n;
      float v = 0.0f;
      if (m < M) {
        const int k = kc0 + kk;
        v = VecIO<T>::to_f32(x[(int64_t)m * K + k]);
        if (ln_g)
          v = ((v - mu_s[m]) - dm_s[m]) * is_s[m] * ln_g[k] + ln_b[k];
      }
      buf[kk * MT + m] = v;
    }
    __syncthreads();
    if (vec)
      sk_chunk<T, MT, true>(B, buf, N, kc0, kc_n, wave, c0, c1, acc);
    else
      sk_chunk<T, MT, false>(B, buf, N, kc0, kc_n, wave, c0, c1, acc);
    __syncthreads();
  }

  // fold the 4 waves' k-interleaved partials (buf is free again)
  if (wave > 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      buf[((wave - 1) * MT + m) * SK_COLS + lane] = acc[m][0];
      buf[((wave - 1) * MT + m) * SK_COLS + 64 + lane] = acc[m][1];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const Epilogue<T> ep{bias, res, N, act_kind};
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m >= M) break;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = j ? c1 : c0;
      if (col >= N) continue;
      float a = acc[m][j];
#pragma unroll
      for (int w = 0; w < 3; ++w)
        a += buf[(w * MT + m) * SK_COLS + j * 64 + lane];
      if (part)
        part[((int64_t)blockIdx.y * M + m) * N + col] = a;
      else
        y[(int64_t)m * N + col] = VecIO<T>::from_f32(ep(a, m, col));
    }
  }
}

// bf16, 4 < M <= 16: the same decomposition with the FMAs on the matrix
// core. Sixteen scalar FMAs per weight element sit at the VALU ceiling at
// HBM rate; v_mfma_f32_32x32x16_bf16 with the batch (zero-padded) as the
// row dimension does them in passing. B is [K][N] but the MFMA B operand
// wants 8 consecutive k per lane for ONE column, so each lane loads its
// column pair from 8 consecutive rows -- straight to VGPRs, 32 lanes x
// 4 B = one full 128-B line per row -- and regroups the 8 dwords in
// registers (two 16-bit selects per
// dword pair) into the operands of two MFMAs: one for the even columns of
// the block, one for the odd ones. No LDS round trip and no transposed
// weight copy. Odd N (rows not dword-aligned) loads single columns
// instead; see the k loop. x is staged as bf16 [m][k] (rows padded 16 B against bank
// conflicts; row 16 is zero and feeds the MFMA's unused rows 16..31), so
// a fused LayerNorm's output is rounded to bf16 here, as the unfused
// layer_norm -> gemm pair rounds it.
constexpr int SKM_COLS = 64;    // columns per block
constexpr int SKM_KC = 1024;    // k rows of x staged per LDS chunk

// even N: the dword holding this lane's column pair, from 8 rows
DEV void skm_load8(const bf16* __restrict__ B, int N, int r0, int r_max,
                   int c0, unsigned (&d)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
    // rows past the slice re-read its last row; x is zero there
    d[j] = *(const unsigned*)&B[(int64_t)min(r0 + j, r_max) * N + c0];
}

// 8 rows of one lane -> the k-contiguous operands of its two columns
DEV void skm_pack(const unsigned (&d)[8], bf16x8& b0, bf16x8& b1) {
  int4v p0, p1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // dword = col c0 | col c0+1 << 16
    p0[i] = (int)((d[2 * i] & 0xFFFFu) | (d[2 * i + 1] << 16));
    p1[i] = (int)((d[2 * i] >> 16) | (d[2 * i + 1] & 0xFFFF0000u));
  }
  b0 = __builtin_bit_cast(bf16x8, p0);
  b1 = __builtin_bit_cast(bf16x8, p1);
}

// odd N: rows are not dword-aligned, so a lane loads ONE column (n0 +
// lane: 64 lanes x 2 B, wave-contiguous) from all 16 rows of a k step
// and packs rows 0..7 and 8..15
DEV void skm_load16(const bf16* __restrict__ B, int N, int r0, int r_max,
                    int c, bf16x8& lo, bf16x8& hi) {
  unsigned d[16];
#pragma unroll
  for (int j = 0; j < 16; ++j)
    d[j] = *(const unsigned short*)&B[(int64_t)min(r0 + j, r_max) * N + c];
  int4v p0, p1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p0[i] = (int)(d[2 * i] | (d[2 * i + 1] << 16));
    p1[i] = (int)(d[8 + 2 * i] | (d[9 + 2 * i] << 16));
  }
  lo = __builtin_bit_cast(bf16x8, p0);
  hi = __builtin_bit_cast(bf16x8, p1);
}

template <bool VEC>
__launch_bounds__(256)
__global__ void k_gemm_skinny_mfma(const bf16* __restrict__ x,
                                   const bf16* __restrict__ B,
                                   const bf16* __restrict__ bias,
                                   const bf16* __restrict__ res,
                                   bf16* __restrict__ y,
                                   float* __restrict__ part,
                                   const float* __restrict__ ln_g,
                                   const float* __restrict__ ln_b,
                                   float ln_eps, int M, int N, int K,
                                   int act_kind) {
  constexpr int XLD = SKM_KC + 8;  // +16 B: rows land 4 banks apart
  __shared__ alignas(16) bf16 xs[17 * XLD];
  __shared__ float red[3 * 16 * 64];
  __shared__ float mu_s[16], is_s[16];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ci = lane & 31;  // column slot (MFMA B lane / output column)
  const int kg = lane >> 5;  // which 8 of a 16-deep k step
  const int n0 = blockIdx.x * SKM_COLS;
  // output columns of the two MFMAs; loads clamp into the row
  const int c0 = VEC ? n0 + 2 * ci : n0 + ci;
  const int c1 = VEC ? c0 + 1 : c0 + 32;
  // the column(s) this lane LOADS: its pair (even N), or n0 + lane (odd
  // N; lanes 0-31 then hold the first MFMA's columns and lanes 32-63 the
  // second's)
  const int lc = VEC ? min(c0, N - 2) : min(n0 + lane, N - 1);
  const int nsplit = gridDim.y;
  const int k_lo = (int)((int64_t)K * blockIdx.y / nsplit);
  const int k_hi = (int)((int64_t)K * (blockIdx.y + 1) / nsplit);

  for (int i = threadIdx.x; i < XLD; i += 256) xs[16 * XLD + i] = f2bf(0.0f);
  if (ln_g) {
    for (int m = wave; m < M; m += 4) {
      // shifted moments, one pass: the shift (the row's first element) is
      // within a few std of the mean, so sq/K - d^2 keeps its digits where
      // raw E[x^2] - mean^2 cancels. The two-pass form of k_gemm_skinny
      // measured +1 us here (8%), and its extra accuracy would be lost in
      // the bf16 staging below anyway.
      const float k0 = bf2f(x[(int64_t)m * K]);
      float sm = 0.0f, sq = 0.0f;
      for (int k = lane; k < K; k += 64) {
        const float v = bf2f(x[(int64_t)m * K + k]) - k0;
        sm += v;
        sq += v * v;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sm += __shfl_xor(sm, off, 64);
        sq += __shfl_xor(sq, off, 64);
      }
      if (lane == 0) {
        const float d = sm / (float)K;  // mean - k0
        mu_s[m] = k0 + d;
        is_s[m] = rsqrtf(fmaxf(sq / (float)K - d * d, 0.0f) + ln_eps);
      }
    }
    __syncthreads();
  }

  f32x16 acc[2] = {};
  const bf16* arow = &xs[(ci < 16 ? ci : 16) * XLD + kg * 8];
  for (int kc0 = k_lo; kc0 < k_hi; kc0 += SKM_KC) {
    const int kc_n = min(SKM_KC, k_hi - kc0);
    const int kc16 = (kc_n + 15) & ~15;
    // stage x[0..16)[kc0 .. kc0 + kc16) as bf16 [m][k], 8 elements per
    // thread and step (one 16-B load where the source allows; element-wise
    // staging serialised ~48 dependent 2-B loads per thread on the vocab
    // head); rows >= M and k >= kc_n are zero
    const int nk8 = kc16 / 8;
    for (int i = threadIdx.x; i < 16 * nk8; i += 256) {
      const int m = i / nk8, kk = (i - m * nk8) * 8;
      float v[8] = {};
      if (m < M) {
        const int k = kc0 + kk;
        const bf16* src = &x[(int64_t)m * K + k];
        if (kk + 8 <= kc_n && aligned16(src)) {
          const Pack16<bf16> p = *(const Pack16<bf16>*)src;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = bf2f(p.e[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (kk + j < kc_n) v[j] = bf2f(src[j]);
        }
        if (ln_g) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (kk + j < kc_n)
              v[j] = (v[j] - mu_s[m]) * is_s[m] * ln_g[k + j] + ln_b[k + j];
        }
      }
      Pack16<bf16> o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o.e[j] = f2bf(v[j]);
      *(Pack16<bf16>*)&xs[m * XLD + kk] = o;
    }
    __syncthreads();
    // this wave's 16-deep k steps: wave, wave + 4, ...
    int ks = wave * 16;
    if constexpr (VEC) {
      // two steps per batch: 16 row loads in flight per lane
      for (; ks + 64 < kc_n; ks += 128) {
        unsigned d[8], e[8];
        skm_load8(B, N, kc0 + ks + kg * 8, k_hi - 1, lc, d);
        skm_load8(B, N, kc0 + ks + 64 + kg * 8, k_hi - 1, lc, e);
        bf16x8 b0, b1;
        const bf16x8 a0 = *(const bf16x8*)&arow[ks];
        const bf16x8 a1 = *(const bf16x8*)&arow[ks + 64];
        skm_pack(d, b0, b1);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[1], 0, 0, 0);
        skm_pack(e, b0, b1);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1], 0, 0, 0);
      }
      for (; ks < kc_n; ks += 64) {
        unsigned d[8];
        skm_load8(B, N, kc0 + ks + kg * 8, k_hi - 1, lc, d);
        bf16x8 b0, b1;
        const bf16x8 a0 = *(const bf16x8*)&arow[ks];
        skm_pack(d, b0, b1);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[1], 0, 0, 0);
      }
    } else {
      // Each lane holds 16 rows of one column, but an MFMA wants both of
      // its k halves (lanes 0-31 / 32-63) on the SAME 32 columns. So every
      // MFMA here is 8 deep: both halves of the A operand read the same 8
      // x values, and the B operand is zero in the half whose lanes hold
      // the other MFMA's columns. Four MFMAs per step instead of two; the
      // matrix core has the room.
      const bf16x8 zero = {};
      const bf16* arow8 = arow - kg * 8;
      for (; ks < kc_n; ks += 64) {
        bf16x8 lo, hi;
        skm_load16(B, N, kc0 + ks, k_hi - 1, lc, lo, hi);
        const bf16x8 a0 = *(const bf16x8*)&arow8[ks];
        const bf16x8 a1 = *(const bf16x8*)&arow8[ks + 8];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a0, kg == 0 ? lo : zero, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a1, kg == 0 ? hi : zero, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a0, kg == 1 ? lo : zero, acc[1], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a1, kg == 1 ? hi : zero, acc[1], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // C/D map of 32x32x16: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2)
  // + 4 * (lane >> 5); rows < 16 live in regs 0..7. Fold the 4 waves.
  if (wave > 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 8; ++r)
        red[((wave - 1) * 16 + e * 8 + r) * 64 + lane] = acc[e][r];
  }
  __syncthreads();
  if (wave != 0) return;
  const Epilogue<bf16> ep{bias, res, N, act_kind};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int col = e ? c1 : c0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int m = (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (m >= M || col >= N) continue;
      float a = acc[e][r];
#pragma unroll
      for (int w = 0; w < 3; ++w) a += red[(w * 16 + e * 8 + r) * 64 + lane];
      if (part)
        part[((int64_t)blockIdx.y * M + m) * N + col] = a;
      else
        y[(int64_t)m * N + col] = f2bf(ep(a, m, col));
    }
  }
}

// fold the K-split partials [nsplit][M*N] in slab order + fused epilogue
template <typename T>
__launch_bounds__(256)
__global__ void k_skinny_fin(const float* __restrict__ part,
                             const T* __restrict__ bias,
                             const T* __restrict__ res, T* __restrict__ y,
                             int64_t mn, int N, int nsplit, int act_kind) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn) return;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  int s = 0;
  for (; s + 4 <= nsplit; s += 4) {
    a0 += part[(int64_t)s * mn + i];
    a1 += part[(int64_t)(s + 1) * mn + i];
    a2 += part[(int64_t)(s + 2) * mn + i];
    a3 += part[(int64_t)(s + 3) * mn + i];
  }
  for (; s < nsplit; ++s) a0 += part[(int64_t)s * mn + i];
  const float a = (a0 + a1) + (a2 + a3);
  y[i] = VecIO<T>::from_f32(
      Epilogue<T>{bias, res, N, act_kind}.at(a, (int)(i % N), i));
}

// bf16 rows past the plain-VALU form's comfort zone go to the MFMA kernel
static bool skinny_use_mfma(DT dt, int M) { return dt == DT::BF16 && M > 4; }

int gemm_skinny_nsplit(DT dt, int M, int N, int K) {
  // fill the chip like gemv_nn1_nsplit: ~2 blocks per CU, slices >= 32 rows
  const int ncb = ceil_div(N, skinny_use_mfma(dt, M) ? SKM_COLS : SK_COLS);
  int ns = std::max(1, std::min(32, 512 / ncb));
  ns = std::min(ns, std::max(1, K / 32));
  return ns;
}

void gemm_skinny_launch(DT dt, const void* x, const void* b, const void* bias,
                        const void* res, void* y, float* part, int nsplit,
                        const float* ln_g, const float* ln_b, float ln_eps,
                        int M, int N, int K, int act_kind, hipStream_t s) {
  const int64_t mn = (int64_t)M * N;
  if (skinny_use_mfma(dt, M)) {
    dim3 g(ceil_div(N, SKM_COLS), nsplit);
    const bool vec = N % 2 == 0 && ((uintptr_t)b % 4) == 0;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, g, dim3(256), 0, s, (const bf16*)x,
                         (const bf16*)b, (const bf16*)bias, (const bf16*)res,
                         (bf16*)y, nsplit > 1 ? part : nullptr, ln_g, ln_b,
                         ln_eps, M, N, K, act_kind);
    };
    if (vec) launch(k_gemm_skinny_mfma<true>);
    else launch(k_gemm_skinny_mfma<false>);
    if (nsplit > 1)
      hipLaunchKernelGGL(k_skinny_fin<bf16>,
                         dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, s,
                         part, (const bf16*)bias, (const bf16*)res, (bf16*)y,
                         mn, N, nsplit, act_kind);
    return;
  }
  dim3 g(ceil_div(N, SK_COLS), nsplit);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    // pair loads need even N (every row then starts pair-aligned)
    const int vec = N % 2 == 0 && ((uintptr_t)b % (2 * sizeof(T))) == 0;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, g, dim3(256), 0, s, (const T*)x, (const T*)b,
                         (const T*)bias, (const T*)res, (T*)y,
                         nsplit > 1 ? part : nullptr, ln_g, ln_b, ln_eps, M, N,
                         K, act_kind, vec);
    };
    if (M <= 2) launch(k_gemm_skinny<T, 2>);
    else if (M <= 4) launch(k_gemm_skinny<T, 4>);
    else if (M <= 8) launch(k_gemm_skinny<T, 8>);
    else launch(k_gemm_skinny<T, 16>);
    if (nsplit > 1)
      hipLaunchKernelGGL(k_skinny_fin<T>, dim3((unsigned)((mn + 255) / 256)),
                         dim3(256), 0, s, part, (const T*)bias, (const T*)res,
                         (T*)y, mn, N, nsplit, act_kind);
  });
}

// Legacy two-kernel K-split matvec (kept for K > GEMV1_MAX_K): fp32
// partials then a finalize pass.
template <typename T>
__launch_bounds__(256)
__global__ void k_gemv_nn_part(const T* __restrict__ x, const T* __restrict__ B,
                               float* __restrict__ ws, int N, int K) {
  int n = blockIdx.x * 256 + threadIdx.x;
  int ks = blockIdx.y, KS = gridDim.y;
  if (n >= N) return;
  int k0 = (int)((int64_t)K * ks / KS), k1 = (int)((int64_t)K * (ks + 1) / KS);
  float a0 = 0.0f, a1 = 0.0f;
  int k = k0;
  for (; k + 2 <= k1; k += 2) {
    a0 += VecIO<T>::to_f32(x[k]) * VecIO<T>::to_f32(B[(int64_t)k * N + n]);
    a1 += VecIO<T>::to_f32(x[k + 1]) *
          VecIO<T>::to_f32(B[(int64_t)(k + 1) * N + n]);
  }
  if (k < k1) a0 += VecIO<T>::to_f32(x[k]) * VecIO<T>::to_f32(B[(int64_t)k * N + n]);
  ws[(int64_t)ks * N + n] = a0 + a1;
}

template <typename T>
__launch_bounds__(256)
__global__ void k_gemv_nn_fin(const float* __restrict__ ws,
                              const T* __restrict__ bias, T* __restrict__ y,
                              int N, int KS, int act_kind) {
  int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float a = 0.0f;
  for (int s = 0; s < KS; ++s) a += ws[(int64_t)s * N + n];
  // no residual on this route (the binding rejects it)
  y[n] = VecIO<T>::from_f32(Epilogue<T>{bias, nullptr, N, act_kind}(a, 0, n));
}

// vector-guaranteed TN gemm (K%V==0, N%V==0, aligned): 3-phase staging --
// addresses (zero-page OOB), all 16B loads, LDS scatter -- keeps RA+RB
// loads in flight where `#pragma unroll 1` serializes to one (see
// k_conv_wgrad_vec).
template <typename T>
__launch_bounds__(THREADS, 3)
__global__ void k_gemm_tn_vec(const T* __restrict__ A, const T* __restrict__ B,
                              float* __restrict__ C,
                              const T* __restrict__ zero16, int M, int N,
                              int K) {
  constexpr int V = 16 / sizeof(T);
  constexpr int RA = BK * (BM / V) / THREADS;
  constexpr int RB = BK * (BN / V) / THREADS;
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];
  const int r0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  using VecT = Pack16<T>;

  for (int k0 = m_begin; k0 < m_end; k0 += BK) {
    // bf16: (8-row group x 4 consecutive m) per thread + in-thread
    // transpose -> ds_write_b64 (see k_conv_wgrad_vec)
    constexpr bool TR = sizeof(T) == 2;
    // lane mapping: consecutive lanes share the m-quad and span the row
    // groups: the 16 lanes' 16B global loads form one contiguous 256B run
    // (the conflict-free same-row/mm-strided write mapping was tried and
    // lost more to broken global coalescing than its bank relief won)
    const int a_rr = TR ? (threadIdx.x & (BM / V - 1)) * V : 0;
    const int a_mm0 = TR ? (threadIdx.x / (BM / V)) * 4 : 0;
    const T* asrc[RA];
#pragma unroll
    for (int it = 0; it < RA; ++it) {
      int mm, rr;
      if constexpr (TR) {
        mm = a_mm0 + it;
        rr = a_rr;
      } else {
        int c = threadIdx.x + it * THREADS;
        mm = c / (BM / V);
        rr = (c % (BM / V)) * V;
      }
      int gm = k0 + mm, gr = r0 + rr;
      asrc[it] = (gm < m_end && gr < K) ? &A[(int64_t)gm * K + gr] : zero16;
    }
    const T* bsrc[RB];
#pragma unroll
    for (int it = 0; it < RB; ++it) {
      int c = threadIdx.x + it * THREADS;
      int mm = c / (BN / V);
      int nn = (c % (BN / V)) * V;
      int gm = k0 + mm, gn = n0 + nn;
      bsrc[it] = (gm < m_end && gn < N) ? &B[(int64_t)gm * N + gn] : zero16;
    }
    VecT va[RA], vb[RB];
#pragma unroll
    for (int it = 0; it < RA; ++it) va[it] = *(const VecT*)asrc[it];
#pragma unroll
    for (int it = 0; it < RB; ++it) vb[it] = *(const VecT*)bsrc[it];
    if constexpr (TR) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        struct alignas(8) H4 { T e[4]; } h;
#pragma unroll
        for (int q = 0; q < 4; ++q) h.e[q] = va[q].e[j];
        *(H4*)&As[lds_off<T>(a_rr + j, a_mm0)] = h;
      }
    } else {
#pragma unroll
      for (int it = 0; it < RA; ++it) {
        int c = threadIdx.x + it * THREADS;
        int mm = c / (BM / V);
        int rr = (c % (BM / V)) * V;
#pragma unroll
        for (int j = 0; j < V; ++j) As[lds_off<T>(rr + j, mm)] = va[it].e[j];
      }
    }
#pragma unroll
    for (int it = 0; it < RB; ++it) {
      int c = threadIdx.x + it * THREADS;
      int mm = c / (BN / V);
      int nn = (c % (BN / V)) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) Bs[lds_off<T>(nn + j, mm)] = vb[it].e[j];
    }
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }

  slab_store(wc, acc, C, r0, n0, K, N);
}

// Where a split reduce puts its result. Elements [0, n0) go to out0 and
// [n0, n) to out1 (a caller without a second destination passes n0 = n), so a
// gradient whose rows belong to two parameters (conv dw rows, then the db
// row) lands in both .grad buffers from the one reduce. acc: the fp32 sum is
// added to the value already at the destination and rounded once. Neither
// changes the order in which the slabs are summed.
template <typename OUT>
struct SplitDst {
  OUT* out0;
  OUT* out1;
  int64_t n0;   // in the kernel's own unit: elements, or groups of 4
  int acc;
  __device__ OUT* at(int64_t i) const {
    return i < n0 ? out0 + i : out1 + (i - n0);
  }
  // group of 4 elements, 4 * sizeof(OUT) aligned at either destination
  __device__ OUT* at4(int64_t i4) const {
    return i4 < n0 ? out0 + 4 * i4 : out1 + 4 * (i4 - n0);
  }
};

template <typename OUT>
__device__ inline void split_store4(const SplitDst<OUT>& d, int64_t i4,
                                    float r0, float r1, float r2, float r3) {
  struct alignas(4 * sizeof(OUT)) O4 { OUT e[4]; };
  O4* p = (O4*)d.at4(i4);
  if (d.acc) {
    O4 g = *p;
    r0 += VecIO<OUT>::to_f32(g.e[0]);
    r1 += VecIO<OUT>::to_f32(g.e[1]);
    r2 += VecIO<OUT>::to_f32(g.e[2]);
    r3 += VecIO<OUT>::to_f32(g.e[3]);
  }
  O4 o;
  o.e[0] = VecIO<OUT>::from_f32(r0);
  o.e[1] = VecIO<OUT>::from_f32(r1);
  o.e[2] = VecIO<OUT>::from_f32(r2);
  o.e[3] = VecIO<OUT>::from_f32(r3);
  *p = o;
}

template <typename OUT>
__global__ void k_splitk_reduce(const float* __restrict__ ws, SplitDst<OUT> d,
                                int z, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float acc = 0.0f;
    for (int s = 0; s < z; ++s) acc += ws[(int64_t)s * n + i];
    OUT* o = d.at(i);
    if (d.acc) acc += VecIO<OUT>::to_f32(*o);
    *o = VecIO<OUT>::from_f32(acc);
  }
}

// float4 variant with 4 independent slab accumulators: the scalar kernel is
// latency-bound (one dependent 4B load per z iteration measured ~1.25 TB/s);
// 16B loads x 4-deep MLP reach the HBM roofline.
template <typename OUT>
__global__ void k_splitk_reduce4(const float4* __restrict__ ws,
                                 SplitDst<OUT> d, int z, int64_t n4) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    float4 a0{0, 0, 0, 0}, a1{0, 0, 0, 0}, a2{0, 0, 0, 0}, a3{0, 0, 0, 0};
    int s = 0;
    for (; s + 4 <= z; s += 4) {
      float4 v0 = ws[(int64_t)s * n4 + i];
      float4 v1 = ws[(int64_t)(s + 1) * n4 + i];
      float4 v2 = ws[(int64_t)(s + 2) * n4 + i];
      float4 v3 = ws[(int64_t)(s + 3) * n4 + i];
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
      a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
      a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
    }
    for (; s < z; ++s) {
      float4 v = ws[(int64_t)s * n4 + i];
      a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
    }
    split_store4(d, i, (a0.x + a1.x) + (a2.x + a3.x),
                 (a0.y + a1.y) + (a2.y + a3.y), (a0.z + a1.z) + (a2.z + a3.z),
                 (a0.w + a1.w) + (a2.w + a3.w));
  }
}

// tall fold for small outputs with many K-slices (e.g. early-conv wgrad:
// n4 a few hundred, z in the hundreds): the flat kernel gets <16 blocks and
// one serial z-chain per thread. Here 256/CPB thread-rows split z per
// column, then an LDS tree folds the rows — same shape as k_slab_fin.
template <typename OUT, int CPB>
__global__ void k_splitk_fold(const float4* __restrict__ ws, SplitDst<OUT> d,
                              int z, int64_t n4) {
  constexpr int RPB = 256 / CPB;
  __shared__ float4 sh[256];
  const int cl = threadIdx.x % CPB;
  const int r = threadIdx.x / CPB;
  const int64_t c = (int64_t)blockIdx.x * CPB + cl;
  float4 a{0.0f, 0.0f, 0.0f, 0.0f};
  if (c < n4)
    for (int sl = r; sl < z; sl += RPB) {
      float4 v = ws[(int64_t)sl * n4 + c];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  sh[r * CPB + cl] = a;
  __syncthreads();
  for (int h = RPB / 2; h > 0; h >>= 1) {
    if (r < h) {
      float4 o = sh[(r + h) * CPB + cl];
      float4 m = sh[r * CPB + cl];
      m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
      sh[r * CPB + cl] = m;
    }
    __syncthreads();
  }
  if (r == 0 && c < n4) {
    float4 m = sh[cl];
    split_store4(d, c, m.x, m.y, m.z, m.w);
  }
}

template <typename OUT>
static void splitk_fold_launch(const float4* ws, SplitDst<OUT> d, int z,
                               int64_t n4, hipStream_t s, int64_t n4_shape) {
#define FOLD_CASE(CPB)                                                    \
  hipLaunchKernelGGL((k_splitk_fold<OUT, CPB>),                           \
                     dim3((unsigned)((n4 + CPB - 1) / CPB)), dim3(256), 0, \
                     s, ws, d, z, n4)
  if (n4_shape >= 128 * 32) FOLD_CASE(32);
  else if (n4_shape >= 128 * 16) FOLD_CASE(16);
  else if (n4_shape >= 128 * 8) FOLD_CASE(8);
  else if (n4_shape >= 128 * 4) FOLD_CASE(4);
  else if (n4_shape >= 128 * 2) FOLD_CASE(2);
  else FOLD_CASE(1);
#undef FOLD_CASE
}

// Whether splitk_reduce_launch can split n elements at n0 between these two
// destinations: always on the scalar kernel (n % 4 != 0); the float4 kernels
// need the boundary on a group of 4 and both destinations aligned to 4
// elements of out_dt. A caller that gets false reduces into one tensor as
// before and copies.
bool splitk_reduce_can_split(int64_t n, int64_t n0, const void* out0,
                             const void* out1, DT out_dt) {
  if ((n & 3) != 0) return true;
  const uintptr_t al = (out_dt == DT::F32 ? 16 : 8) - 1;
  return (n0 & 3) == 0 && ((uintptr_t)out0 & al) == 0 &&
         ((uintptr_t)out1 & al) == 0;
}

// n_shape (default n): the element count the kernel and its fold width are
// chosen for. A caller that appends rows to an output passes the original
// size, so the original elements keep their summation order bit for bit.
// out1 / n0 / accumulate: see SplitDst (out1 == nullptr: everything to out).
void splitk_reduce_launch(const float* ws, void* out, DT out_dt, int z,
                          int64_t n, hipStream_t s, int64_t n_shape,
                          void* out1, int64_t n0, bool accumulate) {
  if (n_shape <= 0) n_shape = n;
  if (!out1) n0 = n;
  // the float4 kernels cannot split anywhere: a caller that did not ask
  // splitk_reduce_can_split first must not get misplaced elements
  if (out1 && (n0 < 0 || n0 > n ||
               !splitk_reduce_can_split(n, n0, out, out1, out_dt)))
    throw std::invalid_argument(
        "splitk_reduce_launch: the two destinations cannot be split here "
        "(boundary or pointer off a group of 4); see splitk_reduce_can_split");
  dispatch_dt(out_dt, [&](auto tag) {
    using OUT = typename decltype(tag)::type;
    const int acc = accumulate ? 1 : 0;
    const SplitDst<OUT> d1{(OUT*)out, (OUT*)out1, n0, acc};
    const SplitDst<OUT> d4{(OUT*)out, (OUT*)out1, n0 >> 2, acc};
    if ((n & 3) == 0 && (n_shape & 3) == 0 && n_shape < 4 * 32768 && z >= 8) {
      // small output x deep z: parallelize over z (see k_splitk_fold)
      splitk_fold_launch((const float4*)ws, d4, z, n >> 2, s, n_shape >> 2);
    } else if ((n & 3) == 0) {
      int64_t n4 = n >> 2;
      int blocks = (int)std::min<int64_t>((n4 + 255) / 256, (int64_t)2048);
      hipLaunchKernelGGL(k_splitk_reduce4<OUT>, dim3(blocks), dim3(256), 0, s,
                         (const float4*)ws, d4, z, n4);
    } else {
      int blocks = (int)std::min<int64_t>((n + 255) / 256, (int64_t)2048);
      hipLaunchKernelGGL(k_splitk_reduce<OUT>, dim3(blocks), dim3(256), 0, s,
                         ws, d1, z, n);
    }
  });
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void gemm_launch(DT dt, const void* a, const void* b, const void* bias,
                 void* c, const void* zero16, const void* resid, int M, int N,
                 int K, bool trans_b, int act_kind, hipStream_t s) {
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const T* A = (const T*)a;
    const T* B = (const T*)b;
    if (M == 1 && trans_b) {  // decode-path matvec
      hipLaunchKernelGGL(k_gemv_nt<T>, dim3(ceil_div(N, 4)), dim3(256), 0, s,
                         A, B, (const T*)bias, (const T*)resid, (T*)c, N, K,
                         act_kind);
      return;
    }
    dim3 grid(ceil_div(M, BM), ceil_div(N, BN));
    // glds stages 16-byte vectors straight from global memory: with
    // trans_b it reads B's rows that way too, so B must be aligned as well
    const bool g = K % vec_elems(dt) == 0 && ptr_aligned16(a) &&
                   (!trans_b || ptr_aligned16(b));
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, A, B,
                         (const T*)bias, (T*)c, (const T*)zero16,
                         (const T*)resid, M, N, K, act_kind);
    };
    if (trans_b && g && K <= 3072)
      launch(k_gemm_nt_db<T>);
    else if (trans_b)
      launch(g ? k_gemm<T, true, true> : k_gemm<T, true, false>);
    else
      launch(g ? k_gemm<T, false, true> : k_gemm<T, false, false>);
  });
}

int gemv_nn_ksplits(int N, int K) {
  int ncb = ceil_div(N, 256);
  int ks = std::max(1, 512 / ncb);
  ks = std::min(ks, std::max(1, K / 16));
  return ks;
}

void gemv_nn_launch(DT dt, const void* x, const void* b, const void* bias,
                    void* y, float* ws, int ks, int N, int K, int act_kind,
                    hipStream_t s) {
  dim3 pg(ceil_div(N, 256), ks);
  dim3 fg(ceil_div(N, 256));
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_gemv_nn_part<T>, pg, dim3(256), 0, s, (const T*)x,
                       (const T*)b, ws, N, K);
    hipLaunchKernelGGL(k_gemv_nn_fin<T>, fg, dim3(256), 0, s, ws,
                       (const T*)bias, (T*)y, N, ks, act_kind);
  });
}

int gemm_tn_zsplits(int M, int N, int K) {
  int base = ceil_div(K, BM) * ceil_div(N, BN);
  int want = 2048;
  int z = base >= want ? 1 : std::min(ceil_div(M, BK), ceil_div(want, base));
  return std::max(z, 1);
}

void gemm_tn_launch(DT dt, const void* a, const void* b, void* c_out,
                    DT out_dt, float* ws, int z, const void* zero16, int M,
                    int N, int K, hipStream_t s) {
  dim3 grid(ceil_div(K, BM), ceil_div(N, BN), z);
  bool direct = z == 1 && out_dt == DT::F32;
  float* target = direct ? (float*)c_out : ws;
  const int V = vec_elems(dt);
  const bool vec = K % V == 0 && N % V == 0 && ptr_aligned16(a) &&
                   ptr_aligned16(b);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (vec)
      hipLaunchKernelGGL(k_gemm_tn_vec<T>, grid, dim3(THREADS), 0, s,
                         (const T*)a, (const T*)b, target, (const T*)zero16,
                         M, N, K);
    else
      hipLaunchKernelGGL(k_gemm_tn<T>, grid, dim3(THREADS), 0, s, (const T*)a,
                         (const T*)b, target, M, N, K);
  });
  if (!direct)
    splitk_reduce_launch(ws, c_out, out_dt, z, (int64_t)K * N, s);
}

// ---------------------------------------------------------------------------
// MFMA layout self-test: single-wave D = A@B for the exact fragment maps
// the tile core assumes (run once on real hardware; asymmetric inputs).
// ---------------------------------------------------------------------------

__global__ void k_mfma_selftest(const bf16* A, const bf16* B, float* D) {
  // A [16][32] row-major, B [32][16] row-major, D [16][16]
  int l = threadIdx.x;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = (__bf16)A[(l & 15) * 32 + (l >> 4) * 8 + j];
    b[j] = (__bf16)B[((l >> 4) * 8 + j) * 16 + (l & 15)];
  }
  f32x4 acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) D[((l >> 4) * 4 + j) * 16 + (l & 15)] = acc[j];
}

__global__ void k_mfma_selftest_f32(const float* A, const float* B, float* D) {
  // A [16][4], B [4][16], D [16][16]
  int l = threadIdx.x;
  float a = A[(l & 15) * 4 + (l >> 4)];
  float b = B[(l >> 4) * 16 + (l & 15)];
  f32x4 acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) D[((l >> 4) * 4 + j) * 16 + (l & 15)] = acc[j];
}

void mfma_selftest_launch(const void* a, const void* b, float* d,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_mfma_selftest, dim3(1), dim3(64), 0, s, (const bf16*)a,
                     (const bf16*)b, d);
}

void mfma_selftest_f32_launch(const float* a, const float* b, float* d,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_mfma_selftest_f32, dim3(1), dim3(64), 0, s, a, b, d);
}

}  // namespace tnn
