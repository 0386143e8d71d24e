// NHWC implicit-GEMM convolution on MFMA: fwd / dgrad / wgrad.
//
// Replaces the reference's cuDNN-frontend conv graphs
// (src/nn/layers_impl/cuda/cudnn_conv2d_ops.cu) and the legacy
// im2col->GEMM path (src/nn/layers_impl/legacy_conv2d_layer.cpp:137) with
// the fused form SURVEY §7 calls for: the im2col gather is folded into the
// GEMM's global->LDS staging, so no im2col buffer ever exists.
//
// GEMM views (row-major):
//   fwd  : y[M=N*OH*OW, Cout] = A[M, K=KH*KW*Cin] @ w[K, Cout]
//   dgrad: dx[M=N*H*W, Cin]   = A'[M, K=KH*KW*Cout] @ w_t[K, Cin]
//   wgrad: dw[K=KH*KW*Cin, Cout] = im2col(x)^T @ dy  (deterministic
//          split-M fp32 slabs + casting reduce -- no atomics)
//
// A-tiles are gathered on the fly: a 16B k-chunk stays within one (kh,kw)
// slice whenever Cin (fwd) / Cout (dgrad) is a multiple of the vector
// width -- which holds for every hot layer, and the python op zero-pads
// narrow-channel inputs (the RGB stem) up to the vector width; a scalar
// gather path remains for the rest.

#include "common.h"
#include "kernels.h"
#include "tile_gemm.h"

namespace tnn {

using namespace tile;

// POW2 resolved at compile time: the ?: form makes hipcc emit BOTH the
// shift and the division and select (measured 2x wgrad regression)
template <bool POW2>
DEV int idiv(int x, const IDiv& f) {
  if constexpr (POW2) return x >> f.lg;
  else if (f.magic)  // mul-shift reciprocal (exact for x < 2^26, see IDiv)
    return (int)(((unsigned long long)(unsigned)x * f.magic) >> f.sh);
  else
    return x / f.d;
}
template <bool POW2>
DEV int imod(int x, const IDiv& f) {
  if constexpr (POW2) return x & (f.d - 1);
  else return x - idiv<POW2>(x, f) * f.d;
}

// kidx -> (kh, kw) via mul-shift reciprocal (exact while kidx * KW < 2^16;
// kidx < KH*KW <= ~169 always). A runtime `%`/`/` by the non-pow2 KW costs
// ~25 VALU per gathered chunk (measured: dgrad 302 -> 446 TF from removing
// the stride modulo; this removes the remaining one).
DEV void kdecode(int kidx, const ConvShape& cs, int& kh, int& kw) {
  kh = (kidx * cs.mkw16) >> 16;
  kw = kidx - kh * cs.KW;
}

// ---------------------------------------------------------------------------
// double-buffered k-loop shared by k_conv_fwd_db and k_conv_dgrad_db, fp32
// and bf16 (all-pow2 shapes, gathered channel count C = 1 << lgC a multiple
// of the 16-byte vector width).
//
// A is gathered from an NHWC tensor with 1 << lgSW columns per image row: tile
// row gm reads pixel (n, p + dh, q + dw), where (n, p, q) depend on the row
// only and the tap (dh, dw, channel c) on the k index only. B is a row-major
// [brows][bstride] matrix read at column bcol(k).
//   row(gm, noff, p, q) -> row < M; noff = element offset of image n
//   tap(gk, dh, dw, c, bcol)   decodes one k index (scalar or per lane)
//   at(p, q, dh, dw, sh, sw) -> pixel valid; (sh, sw) = source pixel
// Staging: a lane's slot in each of its DMA instructions never moves, so the
// row decode, row validity and base pointers are computed once, before the
// loop. With C % BK == 0 a chunk lies in one (kh,kw) slice: its tap is
// decoded once, in scalar registers. Narrower C (and with it the ragged last
// chunk) decodes per instruction. Invalid lanes select the zero page
// branch-free: the address is computed and dropped.
// K: no DMA ever reads at or past k index K. K == 0 is a real case (a
// stride-2 parity class of a 1x1 kernel has no tap): nothing is staged and
// acc stays zero. On the one-tap-per-chunk path K is a multiple of BK, so the
// chunk-level test kk0 < K covers every lane; the per-instruction path tests
// each lane's own k index.
// Sync: counted vmcnt + raw s_barrier only. The bf16 fragment reads are
// asm-issued (tile_gemm.h, rm_frag_issue), so the next chunk's DMAs stay in
// flight under this chunk's MFMAs; the fp32 reads stay visible to the
// compiler, which drains the DMAs before them as it always did. Chunk, k-step
// and MFMA order are those of the single-buffer kernels: the accumulators are
// bitwise the same.
template <bool DB, typename T, typename RowFn, typename TapFn, typename AtFn>
DEV void conv_db_kloop(T* As0, T* As1, T* Bs0, T* Bs1,
                       const WaveCoord& wc, f32x4 acc[FM][FN],
                       const T* __restrict__ asrc, int lgSW, int lgC,
                       const T* __restrict__ bsrc, int64_t bstride,
                       int brows, int m0, int n0, int K,
                       const T* __restrict__ zero16, RowFn&& row,
                       TapFn&& tap, AtFn&& at) {
  constexpr int NA = glds_count<T, BM>();   // A glds per wave
  constexpr int NB = glds_count<T, BN>();   // B glds per wave
  constexpr int NPER = NA + NB;
  const int wid = __builtin_amdgcn_readfirstlane(wc.wid);
  const bool uni = lgC >= 6;   // C % BK == 0: one tap per chunk

  const T* ab[NA];
  int ap[NA], aq[NA];          // ap very negative: row past M, never valid
  const T* bb[NB];
  bool bok[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int j = wid * NA + i;
    int64_t noff;
    int p, q;
    const bool ok = row(m0 + glds_row<T>(j, wc.lane), noff, p, q);
    ab[i] = asrc + noff + (uni ? glds_kk<T>(j, wc.lane) : 0);
    ap[i] = ok ? p : -(1 << 28);
    aq[i] = q;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int j = wid * NB + i;
    const int gn = n0 + glds_row<T>(j, wc.lane);
    bok[i] = gn < brows;
    bb[i] = bsrc + (int64_t)gn * bstride + (uni ? glds_kk<T>(j, wc.lane) : 0);
  }

  auto a_ptr = [&](int i, int dh, int dw, int c, bool& ok) {
    int sh, sw;
    ok = at(ap[i], aq[i], dh, dw, sh, sw);
    const unsigned pix = ((unsigned)sh << lgSW) + (unsigned)sw;
    return ab[i] + (int)((pix << lgC) + (unsigned)c);
  };
  auto stage = [&](int t, T* a_img, T* b_img) {
    const int kk0 = t * BK;
    if (uni) {
      int dh, dw, c, bcol;
      tap(kk0, dh, dw, c, bcol);
      const bool kin = kk0 < K;   // wave-uniform
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        bool ok;
        const T* p = a_ptr(i, dh, dw, c, ok);
        glds_issue(a_img, wid * NA + i, (ok & kin) ? p : zero16);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i)
        glds_issue(b_img, wid * NB + i,
                   (bok[i] & kin) ? bb[i] + bcol : zero16);
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int gk = kk0 + glds_kk<T>(wid * NA + i, wc.lane);
        int dh, dw, c, bcol;
        tap(gk, dh, dw, c, bcol);
        bool ok;
        const T* p = a_ptr(i, dh, dw, c, ok);
        glds_issue(a_img, wid * NA + i, (ok & (gk < K)) ? p : zero16);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int gk = kk0 + glds_kk<T>(wid * NB + i, wc.lane);
        int dh, dw, c, bcol;
        tap(gk, dh, dw, c, bcol);
        glds_issue(b_img, wid * NB + i,
                   (bok[i] & (gk < K)) ? bb[i] + bcol : zero16);
      }
    }
  };
  // chunk t sits in (a_cur, b_cur); the next one streams into the other
  // buffer under this chunk's MFMAs
  const int nch = (K + BK - 1) / BK;
  if (nch == 0) return;
  auto compute = [&](const T* a_img, const T* b_img) {
    if constexpr (sizeof(T) == 2)
      mfma_compute_tile_nofence(a_img, b_img, wc, acc);
    else
      mfma_compute_tile(a_img, b_img, wc, acc);
  };
  auto step = [&](int t, T* a_cur, T* b_cur, T* a_nxt, T* b_nxt) {
    if (t + 1 < nch) {
      stage(t + 1, a_nxt, b_nxt);
      wait_vmcnt<NPER>();   // chunk t landed; t+1 stays in flight
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    compute(a_cur, b_cur);
    __builtin_amdgcn_s_barrier();   // cur free for the t+2 stage
  };
  if constexpr (DB) {
    stage(0, As0, Bs0);
    for (int t = 0; t < nch; t += 2) {
      step(t, As0, Bs0, As1, Bs1);
      if (t + 1 < nch) step(t + 1, As1, Bs1, As0, Bs0);
    }
  } else {
    // single buffer (As1 / Bs1 unused): half the LDS, twice the resident
    // blocks, no overlap inside a block
    for (int t = 0; t < nch; ++t) {
      stage(t, As0, Bs0);
      wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      compute(As0, Bs0);
      __builtin_amdgcn_s_barrier();
    }
  }
}

// ---------------------------------------------------------------------------
// double-buffered pure-glds forward: both operands DMA straight to LDS
// (weights pre-transposed to [Cout, K] so B rows are k-contiguous), the
// next chunk's DMAs overlap the current chunk's MFMAs. Counted
// s_waitcnt vmcnt + raw s_barrier per the CDNA4 glds idiom -- a
// __syncthreads() here would drain the in-flight next-chunk DMAs.
template <typename T, bool POW2, bool STATS, bool DB>
DEV void conv_fwd_glds_tile(const T* __restrict__ X,
                            const T* __restrict__ WT2,
                            const float* __restrict__ bias_f32,
                            const T* __restrict__ bias_t, T* __restrict__ Y,
                            const T* __restrict__ zero16, const ConvShape& cs,
                            int act_kind, float* __restrict__ stats) {
  const int M = cs.N * cs.OH * cs.OW;
  const int K = cs.KH * cs.KW * cs.Cin;
  int tm_, tn_;
  // grouped tile ordering when the gathered activation stream exceeds
  // the 256 MiB L3 across its Cout/BN re-reads (see tile_gemm.h)
  if ((int64_t)cs.N * cs.OH * cs.OW * (cs.KH * cs.KW * cs.Cin) >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tm_, tn_);
  else {
    tm_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  auto row = [&](int gm, int64_t& noff, int& p, int& q) {
    const int n = gm >> cs.d_ohow.lg;
    const int rem = gm & (cs.OH * cs.OW - 1);
    p = (rem >> cs.d_ow.lg) * cs.SH - cs.PH;
    q = (rem & (cs.OW - 1)) * cs.SW - cs.PW;
    noff = (int64_t)n << (cs.d_hw.lg + cs.d_cin.lg);
    return gm < M;
  };
  auto tap = [&](int gk, int& dh, int& dw, int& c, int& bcol) {
    kdecode(gk >> cs.d_cin.lg, cs, dh, dw);
    c = gk & (cs.Cin - 1);
    bcol = gk;
  };
  auto at = [&](int p, int q, int dh, int dw, int& ih, int& iw) {
    ih = p + dh;
    iw = q + dw;
    return (unsigned)ih < (unsigned)cs.H && (unsigned)iw < (unsigned)cs.W;
  };
  if constexpr (DB) {
    // one LDS object per buffer, named statically in the 2x-unrolled loop
    __shared__ alignas(16) T As0[BM * BK], As1[BM * BK];
    __shared__ alignas(16) T Bs0[BN * BK], Bs1[BN * BK];
    conv_db_kloop<true>(As0, As1, Bs0, Bs1, wc, acc, X, cs.d_w.lg,
                        cs.d_cin.lg, WT2, (int64_t)K, cs.Cout, m0, n0, K,
                        zero16, row, tap, at);
  } else {
    __shared__ alignas(16) T As0[BM * BK], Bs0[BN * BK];
    conv_db_kloop<false>(As0, As0, Bs0, Bs0, wc, acc, X, cs.d_w.lg,
                         cs.d_cin.lg, WT2, (int64_t)K, cs.Cout, m0, n0, K,
                         zero16, row, tap, at);
  }

  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < cs.Cout) {
      if (bias_f32) v += bias_f32[col];
      if (bias_t) v += VecIO<T>::to_f32(bias_t[col]);
      if (act_kind != ACT_LINEAR) v = act_apply(v, act_kind);
      Y[(int64_t)row * cs.Cout + col] = VecIO<T>::from_f32(v);
    }
  });

  if constexpr (STATS) {
    // per-channel sum/sumsq of the tile straight from the accumulators
    // (post-bias, linear act only): saves the BN stats pass's full read
    // of y. C/D fragment col = lane&15; lanes {l, l+16, l+32, l+48} share
    // a column -> two shfl_xor folds, then one atomic per (block, col).
    float* ssum = stats;
    float* ssumsq = stats + cs.Cout;
    const int cr = (wc.lane >> 4) * 4;
    const int cc = wc.lane & 15;
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      int col = n0 + wc.wcol0 + fn * 16 + cc;
      float bias = 0.0f;
      if (col < cs.Cout) {
        if (bias_f32) bias = bias_f32[col];
        if (bias_t) bias = VecIO<T>::to_f32(bias_t[col]);
      }
      float s = 0.0f, ss = 0.0f;
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int row = m0 + wc.wrow0 + fm * 16 + cr + j;
          if (row < M && col < cs.Cout) {
            float v = acc[fm][fn][j] + bias;
            s += v;
            ss += v * v;
          }
        }
      s += __shfl_xor(s, 16, 64);
      ss += __shfl_xor(ss, 16, 64);
      s += __shfl_xor(s, 32, 64);
      ss += __shfl_xor(ss, 32, 64);
      if (wc.lane < 16 && col < cs.Cout) {
        atomicAdd(&ssum[col], s);
        atomicAdd(&ssumsq[col], ss);
      }
    }
  }
}

template <typename T, bool POW2, bool STATS = false>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd_db(const T* __restrict__ X,
                              const T* __restrict__ WT2,
                              const float* __restrict__ bias_f32,
                              const T* __restrict__ bias_t, T* __restrict__ Y,
                              const T* __restrict__ zero16, ConvShape cs,
                              int act_kind, float* __restrict__ stats) {
  conv_fwd_glds_tile<T, POW2, STATS, true>(X, WT2, bias_f32, bias_t, Y, zero16,
                                           cs, act_kind, stats);
}

// the same tile on one LDS buffer pair for the long k-loops past the double
// buffer's gate: 24 KB LDS, 72 VGPR + 32 AGPR, register-limited at 4 blocks
// per CU (the double buffer: 3)
template <bool STATS>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd_sb(const bf16* __restrict__ X,
                              const bf16* __restrict__ WT2,
                              const bf16* __restrict__ bias_t,
                              bf16* __restrict__ Y,
                              const bf16* __restrict__ zero16, ConvShape cs,
                              int act_kind, float* __restrict__ stats) {
  conv_fwd_glds_tile<bf16, true, STATS, false>(X, WT2, nullptr, bias_t, Y,
                                               zero16, cs, act_kind, stats);
}

// ---------------------------------------------------------------------------
template <typename T, bool POW2, bool GLDS>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd(const T* __restrict__ X, const T* __restrict__ Wt,
                           const float* __restrict__ bias_f32,
                           const T* __restrict__ bias_t, T* __restrict__ Y,
                           const T* __restrict__ zero16, ConvShape cs,
                           int act_kind) {
  constexpr int V = 16 / sizeof(T);
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];

  const int M = cs.N * cs.OH * cs.OW;
  const int K = cs.KH * cs.KW * cs.Cin;
  int tm_, tn_;
  // grouped tile ordering when the gathered activation stream exceeds
  // the 256 MiB L3 across its Cout/BN re-reads (see tile_gemm.h)
  if ((int64_t)cs.N * cs.OH * cs.OW * (cs.KH * cs.KW * cs.Cin) >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tm_, tn_);
  else {
    tm_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  using VecT = Pack16<T>;

  // fused-im2col source address for a 16B chunk (row, kk elem), or the
  // zero page when the chunk is out of image/padding/tail range; only
  // called on the GLDS path where Cin % V == 0 guarantees one (kh,kw)
  // slice per chunk.
  auto a_src = [&](int k0, int rl, int kk) -> const T* {
    int gm = m0 + rl, gk = k0 + kk;
    if (gm >= M || gk >= K) return zero16;
    int n = idiv<POW2>(gm, cs.d_ohow);
    int rem = gm - n * (cs.OH * cs.OW);
    int oh = idiv<POW2>(rem, cs.d_ow), ow = rem - oh * cs.OW;
    int ci = imod<POW2>(gk, cs.d_cin);
    int kidx = idiv<POW2>(gk, cs.d_cin);
    int kh, kw;
    kdecode(kidx, cs, kh, kw);
    int ih = oh * cs.SH - cs.PH + kh;
    int iw = ow * cs.SW - cs.PW + kw;
    if (ih < 0 || ih >= cs.H || iw < 0 || iw >= cs.W) return zero16;
    return &X[(((int64_t)n * cs.H + ih) * cs.W + iw) * cs.Cin + ci];
  };

  for (int k0 = 0; k0 < K; k0 += BK) {
    if constexpr (GLDS) {
      glds_stage_a<T>(As, wc, [&](int rl, int kk) { return a_src(k0, rl, kk); });
    } else {
    // ---- stage A: im2col gather ----
#pragma unroll
    for (int c = threadIdx.x; c < BM * (BK / V); c += THREADS) {
      int row = c / (BK / V);
      int kk = (c % (BK / V)) * V;
      int gm = m0 + row, gk = k0 + kk;
      VecT v = {};
      if (gm < M && gk < K) {
        int n = idiv<POW2>(gm, cs.d_ohow);
        int rem = gm - n * (cs.OH * cs.OW);
        int oh = idiv<POW2>(rem, cs.d_ow), ow = rem - oh * cs.OW;
        int ci = imod<POW2>(gk, cs.d_cin);
        int kidx = idiv<POW2>(gk, cs.d_cin);
        int kh, kw;
    kdecode(kidx, cs, kh, kw);
        if (ci + V <= cs.Cin && gk + V <= K && (cs.Cin % V) == 0 &&
            aligned16(X)) {
          int ih = oh * cs.SH - cs.PH + kh;
          int iw = ow * cs.SW - cs.PW + kw;
          if (ih >= 0 && ih < cs.H && iw >= 0 && iw < cs.W)
            v = *(const VecT*)&X[(((int64_t)n * cs.H + ih) * cs.W + iw) *
                                     cs.Cin + ci];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            int k = gk + j;
            if (k < K) {
              int cij = imod<POW2>(k, cs.d_cin);
              int kj = idiv<POW2>(k, cs.d_cin);
              int kwj = kj % cs.KW, khj = kj / cs.KW;
              int ih = oh * cs.SH - cs.PH + khj;
              int iw = ow * cs.SW - cs.PW + kwj;
              if (ih >= 0 && ih < cs.H && iw >= 0 && iw < cs.W)
                v.e[j] = X[(((int64_t)n * cs.H + ih) * cs.W + iw) * cs.Cin + cij];
            }
          }
        }
      }
      *(VecT*)&As[lds_off<T>(row, kk)] = v;
    }
    }
    // ---- stage B (weights [K, Cout]) -> Bs[n][k] scatter-transpose ----
#pragma unroll
    for (int c = threadIdx.x; c < BK * (BN / V); c += THREADS) {
      int kk = c / (BN / V);
      int nn = (c % (BN / V)) * V;
      int gk = k0 + kk, gn = n0 + nn;
      VecT v = {};
      if (gk < K) {
        const T* src = &Wt[(int64_t)gk * cs.Cout + gn];
        if (gn + V <= cs.Cout && aligned16(src)) {
          v = *(const VecT*)src;
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (gn + j < cs.Cout) v.e[j] = Wt[(int64_t)gk * cs.Cout + gn + j];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        Bs[lds_off<T>(nn + j, kk)] = v.e[j];
    }
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }

  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < cs.Cout) {
      if (bias_f32) v += bias_f32[col];
      if (bias_t) v += VecIO<T>::to_f32(bias_t[col]);
      if (act_kind != ACT_LINEAR) v = act_apply(v, act_kind);
      Y[(int64_t)row * cs.Cout + col] = VecIO<T>::from_f32(v);
    }
  });
}

// ---------------------------------------------------------------------------
// dgrad: dx[n,ih,iw,ci] = sum_{kh,kw,co} dy[n,oh,ow,co] * w[kh,kw,ci,co]
// with oh = (ih+PH-kh)/SH when divisible. Wt here is the transposed weight
// [KH,KW,Cout,Cin] so B rows are k=(kh,kw,co) with ci contiguous.
// ---------------------------------------------------------------------------
template <typename T, bool POW2, bool GLDS, bool S2 = false, bool S1 = false>
__launch_bounds__(THREADS)
__global__ void k_conv_dgrad(const T* __restrict__ DY, const T* __restrict__ WT,
                             T* __restrict__ DX, const T* __restrict__ zero16,
                             ConvShape cs) {
  constexpr int V = 16 / sizeof(T);
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];

  // S2: stride-2 parity decomposition. blockIdx.z selects the
  // (ih%2, iw%2) class so every (kh,kw) visited satisfies the stride
  // divisibility test by construction -- the generic kernel at stride 2
  // burns 3/4 of its MFMAs multiplying gathered zeros. The launcher
  // rewrites cs.d_hw/d_w to the per-class (Hc*Wc, Wc) divisors.
  const int cls_a = S2 ? ((int)blockIdx.z >> 1) : 0;
  const int cls_b = S2 ? ((int)blockIdx.z & 1) : 0;
  const int start_h = S2 ? ((cls_a + cs.PH) & 1) : 0;
  const int start_w = S2 ? ((cls_b + cs.PW) & 1) : 0;
  const int nkh = S2 ? ((cs.KH - start_h + 1) >> 1) : cs.KH;
  const int nkw = S2 ? ((cs.KW - start_w + 1) >> 1) : cs.KW;
  const int Hc = S2 ? (cs.H >> 1) : cs.H;
  const int Wc = S2 ? (cs.W >> 1) : cs.W;
  const int M = cs.N * Hc * Wc;
  const int K = nkh * nkw * cs.Cout;
  int tm_, tn_;
  // grouped tile ordering when the gathered activation stream exceeds
  // the 256 MiB L3 across its Cout/BN re-reads (see tile_gemm.h)
  if ((int64_t)cs.N * cs.OH * cs.OW * (cs.KH * cs.KW * cs.Cin) >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tm_, tn_);
  else {
    tm_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  using VecT = Pack16<T>;

  auto a_src = [&](int k0, int rl, int kk) -> const T* {
    int gm = m0 + rl, gk = k0 + kk;
    if (gm >= M || gk >= K) return zero16;
    int n = idiv<POW2>(gm, cs.d_hw);
    int rem = gm - n * (Hc * Wc);
    int ih = idiv<POW2>(rem, cs.d_w), iw = rem - ih * Wc;
    int co = imod<POW2>(gk, cs.d_cout);
    int kidx = idiv<POW2>(gk, cs.d_cout);
    if constexpr (S2) {
      ih = 2 * ih + cls_a;
      iw = 2 * iw + cls_b;
      int kwi = kidx & (nkw - 1);              // nkw is 1 or 2
      int khi = nkw == 2 ? (kidx >> 1) : kidx;
      int kh = start_h + 2 * khi, kw = start_w + 2 * kwi;
      int th = ih + cs.PH - kh, tw = iw + cs.PW - kw;
      if (th < 0 || tw < 0) return zero16;
      int oh = th >> 1, ow = tw >> 1;          // divisible by construction
      if (oh >= cs.OH || ow >= cs.OW) return zero16;
      return &DY[(((int64_t)n * cs.OH + oh) * cs.OW + ow) * cs.Cout + co];
    } else {
      int kh, kw;
    kdecode(kidx, cs, kh, kw);
      int th = ih + cs.PH - kh, tw = iw + cs.PW - kw;
      if constexpr (S1) {  // stride 1: no divisibility test, oh == th
        if (th < 0 || tw < 0 || th >= cs.OH || tw >= cs.OW) return zero16;
        return &DY[(((int64_t)n * cs.OH + th) * cs.OW + tw) * cs.Cout + co];
      } else {
        if (th < 0 || tw < 0 || th % cs.SH || tw % cs.SW) return zero16;
        int oh = th / cs.SH, ow = tw / cs.SW;
        if (oh >= cs.OH || ow >= cs.OW) return zero16;
        return &DY[(((int64_t)n * cs.OH + oh) * cs.OW + ow) * cs.Cout + co];
      }
    }
  };

  for (int k0 = 0; k0 < K; k0 += BK) {
    if constexpr (GLDS) {
      glds_stage_a<T>(As, wc, [&](int rl, int kk) { return a_src(k0, rl, kk); });
    } else {
    // ---- stage A: gather dy with stride/padding inversion ----
#pragma unroll
    for (int c = threadIdx.x; c < BM * (BK / V); c += THREADS) {
      int row = c / (BK / V);
      int kk = (c % (BK / V)) * V;
      int gm = m0 + row, gk = k0 + kk;
      VecT v = {};
      if (gm < M && gk < K) {
        int n = idiv<POW2>(gm, cs.d_hw);
        int rem = gm - n * (cs.H * cs.W);
        int ih = idiv<POW2>(rem, cs.d_w), iw = rem - ih * cs.W;
        int co = imod<POW2>(gk, cs.d_cout);
        int kidx = idiv<POW2>(gk, cs.d_cout);
        int kh, kw;
    kdecode(kidx, cs, kh, kw);
        auto gather_one = [&](int khj, int kwj, int coj) -> T {
          int th = ih + cs.PH - khj, tw = iw + cs.PW - kwj;
          if (th < 0 || tw < 0 || th % cs.SH || tw % cs.SW) return T(0.0f);
          int oh = th / cs.SH, ow = tw / cs.SW;
          if (oh >= cs.OH || ow >= cs.OW) return T(0.0f);
          return DY[(((int64_t)n * cs.OH + oh) * cs.OW + ow) * cs.Cout + coj];
        };
        if (co + V <= cs.Cout && gk + V <= K && (cs.Cout % V) == 0 &&
            aligned16(DY)) {
          int th = ih + cs.PH - kh, tw = iw + cs.PW - kw;
          if (th >= 0 && tw >= 0 && th % cs.SH == 0 && tw % cs.SW == 0) {
            int oh = th / cs.SH, ow = tw / cs.SW;
            if (oh < cs.OH && ow < cs.OW)
              v = *(const VecT*)&DY[(((int64_t)n * cs.OH + oh) * cs.OW + ow) *
                                        cs.Cout + co];
          }
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            int k = gk + j;
            if (k < K) {
              int coj = imod<POW2>(k, cs.d_cout);
              int kj = idiv<POW2>(k, cs.d_cout);
              v.e[j] = gather_one(kj / cs.KW, kj % cs.KW, coj);
            }
          }
        }
      }
      *(VecT*)&As[lds_off<T>(row, kk)] = v;
    }
    }
    // ---- stage B (w_t [KH*KW*Cout, Cin]) -> Bs[ci][k] ----
#pragma unroll
    for (int c = threadIdx.x; c < BK * (BN / V); c += THREADS) {
      int kk = c / (BN / V);
      int nn = (c % (BN / V)) * V;
      int gk = k0 + kk, gn = n0 + nn;
      VecT v = {};
      if (gk < K) {
        int64_t wrow = gk;
        if constexpr (S2) {
          // compacted (khi,kwi,co) -> full (kh*KW+kw)*Cout+co row of WT
          int co = imod<POW2>(gk, cs.d_cout);
          int kidx = idiv<POW2>(gk, cs.d_cout);
          int kwi = kidx & (nkw - 1);
          int khi = nkw == 2 ? (kidx >> 1) : kidx;
          wrow = (int64_t)((start_h + 2 * khi) * cs.KW + start_w + 2 * kwi) *
                     cs.Cout + co;
        }
        const T* src = &WT[wrow * cs.Cin + gn];
        if (gn + V <= cs.Cin && aligned16(src)) {
          v = *(const VecT*)src;
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (gn + j < cs.Cin) v.e[j] = src[j];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        Bs[lds_off<T>(nn + j, kk)] = v.e[j];
    }
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }

  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < cs.Cin) {
      int64_t pix = row;
      if constexpr (S2) {
        int n = idiv<POW2>(row, cs.d_hw);
        int rem = row - n * (Hc * Wc);
        int ihp = idiv<POW2>(rem, cs.d_w);
        int ih = 2 * ihp + cls_a, iw = 2 * (rem - ihp * Wc) + cls_b;
        pix = ((int64_t)n * cs.H + ih) * cs.W + iw;
      }
      DX[pix * cs.Cin + col] = VecIO<T>::from_f32(v);
    }
  });
}

// ---------------------------------------------------------------------------
// double-buffered pure-glds dgrad (see k_conv_fwd_db): the weight comes
// pre-transposed to [Cin, KH*KW*Cout] so B rows are k-contiguous; with S2
// the compacted parity-class k index remaps into the full column space.
template <typename T, bool POW2, bool S2 = false, bool S1 = false>
__launch_bounds__(THREADS)
__global__ void k_conv_dgrad_db(const T* __restrict__ DY,
                                const T* __restrict__ WT2D,
                                T* __restrict__ DX,
                                const T* __restrict__ zero16, ConvShape cs) {
  const int cls_a = S2 ? ((int)blockIdx.z >> 1) : 0;
  const int cls_b = S2 ? ((int)blockIdx.z & 1) : 0;
  const int start_h = S2 ? ((cls_a + cs.PH) & 1) : 0;
  const int start_w = S2 ? ((cls_b + cs.PW) & 1) : 0;
  const int nkh = S2 ? ((cs.KH - start_h + 1) >> 1) : cs.KH;
  const int nkw = S2 ? ((cs.KW - start_w + 1) >> 1) : cs.KW;
  const int Hc = S2 ? (cs.H >> 1) : cs.H;
  const int Wc = S2 ? (cs.W >> 1) : cs.W;
  const int M = cs.N * Hc * Wc;
  const int K = nkh * nkw * cs.Cout;
  const int KFULL = cs.KH * cs.KW * cs.Cout;
  int tm_, tn_;
  // grouped tile ordering when the gathered activation stream exceeds
  // the 256 MiB L3 across its Cout/BN re-reads (see tile_gemm.h)
  if ((int64_t)cs.N * cs.OH * cs.OW * (cs.KH * cs.KW * cs.Cin) >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tm_, tn_);
  else {
    tm_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  // one LDS object per buffer, named statically in the 2x-unrolled k-loop
  __shared__ alignas(16) T As0[BM * BK], As1[BM * BK];
  __shared__ alignas(16) T Bs0[BN * BK], Bs1[BN * BK];
  conv_db_kloop<true>(
      As0, As1, Bs0, Bs1, wc, acc, DY, cs.d_ow.lg, cs.d_cout.lg, WT2D,
      (int64_t)KFULL, cs.Cin, m0, n0, K, zero16,
      // d_hw / d_w hold the per-class (Hc*Wc, Wc) divisors under S2
      [&](int gm, int64_t& noff, int& p, int& q) {
        const int n = gm >> cs.d_hw.lg;
        const int rem = gm & (Hc * Wc - 1);
        int ih = rem >> cs.d_w.lg, iw = rem & (Wc - 1);
        if constexpr (S2) {
          // th = ih + PH - kh is even by construction: oh = p - khi
          p = (2 * ih + cls_a + cs.PH - start_h) >> 1;
          q = (2 * iw + cls_b + cs.PW - start_w) >> 1;
        } else {
          p = ih + cs.PH;
          q = iw + cs.PW;
        }
        noff = (int64_t)n << (cs.d_ohow.lg + cs.d_cout.lg);
        return gm < M;
      },
      [&](int gk, int& dh, int& dw, int& c, int& bcol) {
        const int kidx = gk >> cs.d_cout.lg;
        c = gk & (cs.Cout - 1);
        if constexpr (S2) {
          // compacted (khi,kwi,co) -> full (kh*KW+kw)*Cout+co column
          const int kwi = kidx & (nkw - 1);              // nkw is 1 or 2
          const int khi = nkw == 2 ? (kidx >> 1) : kidx;
          dh = khi;
          dw = kwi;
          bcol = (((start_h + 2 * khi) * cs.KW + start_w + 2 * kwi)
                  << cs.d_cout.lg) + c;
        } else {
          kdecode(kidx, cs, dh, dw);
          bcol = gk;
        }
      },
      [&](int p, int q, int dh, int dw, int& oh, int& ow) {
        const int th = p - dh, tw = q - dw;
        if constexpr (S2 || S1) {
          oh = th;
          ow = tw;
          return (unsigned)oh < (unsigned)cs.OH &&
                 (unsigned)ow < (unsigned)cs.OW;
        } else {
          oh = th / cs.SH;
          ow = tw / cs.SW;
          return th >= 0 && tw >= 0 && oh * cs.SH == th &&
                 ow * cs.SW == tw && oh < cs.OH && ow < cs.OW;
        }
      });

  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < cs.Cin) {
      int64_t pix = row;
      if constexpr (S2) {
        int n = idiv<POW2>(row, cs.d_hw);
        int rem = row - n * (Hc * Wc);
        int ihp = idiv<POW2>(rem, cs.d_w);
        int ih = 2 * ihp + cls_a, iw = 2 * (rem - ihp * Wc) + cls_b;
        pix = ((int64_t)n * cs.H + ih) * cs.W + iw;
      }
      DX[pix * cs.Cin + col] = VecIO<T>::from_f32(v);
    }
  });
}

// ---------------------------------------------------------------------------
// wgrad: dw[(kh,kw,ci), co] += sum_m x_gather * dy ; fp32 atomics over
// grid.z m-slices.
// ---------------------------------------------------------------------------
template <typename T, bool POW2>
__launch_bounds__(THREADS, 3)  // cap VGPRs: unconstrained allocation hit 221-256 VGPR = 1-2 waves/SIMD
__global__ void k_conv_wgrad(const T* __restrict__ X, const T* __restrict__ DY,
                             float* __restrict__ DW, ConvShape cs,
                             int bias_row) {
  constexpr int V = 16 / sizeof(T);
  __shared__ alignas(16) T As[BM * BK];  // rows = (kh,kw,ci), k = m
  __shared__ alignas(16) T Bs[BN * BK];  // rows = co, k = m

  const int M = cs.N * cs.OH * cs.OW;         // reduction dim
  const int Kout = cs.KH * cs.KW * cs.Cin;    // output rows
  int tr_, tn_;
  // same grouped ordering: the gathered-x A operand [Kout, M] is
  // re-read gridDim.y times without it
  if ((int64_t)(cs.KH * cs.KW * cs.Cin) * cs.N * cs.OH * cs.OW >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tr_, tn_);
  else {
    tr_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int r0 = tr_ * BM;
  const int n0 = tn_ * BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  // bias gradient: tile-row 0 (one block per n-tile and split) also sums
  // the columns of its dy tiles and writes them as slab row Kout
  const bool colsum = bias_row && tr_ == 0;
  float bsum = 0.0f;
  using VecT = Pack16<T>;

  for (int k0 = m_begin; k0 < m_end; k0 += BK) {
    // ---- stage A^T: x rows ci-contiguous, scatter into As[ko][m] ----
#pragma unroll 1  // full unroll quadruples live address state (spills)
    for (int c = threadIdx.x; c < BK * (BM / V); c += THREADS) {
      int mm = c / (BM / V);
      int rr = (c % (BM / V)) * V;
      int gm = k0 + mm;
      int gr = r0 + rr;
      VecT v = {};
      if (gm < m_end && gr < Kout) {
        int n = idiv<POW2>(gm, cs.d_ohow);
        int rem = gm - n * (cs.OH * cs.OW);
        int oh = idiv<POW2>(rem, cs.d_ow), ow = rem - oh * cs.OW;
        int ci = imod<POW2>(gr, cs.d_cin);
        int kidx = idiv<POW2>(gr, cs.d_cin);
        int kh, kw;
    kdecode(kidx, cs, kh, kw);
        if (ci + V <= cs.Cin && gr + V <= Kout && (cs.Cin % V) == 0 &&
            aligned16(X)) {
          int ih = oh * cs.SH - cs.PH + kh;
          int iw = ow * cs.SW - cs.PW + kw;
          if (ih >= 0 && ih < cs.H && iw >= 0 && iw < cs.W)
            v = *(const VecT*)&X[(((int64_t)n * cs.H + ih) * cs.W + iw) *
                                     cs.Cin + ci];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            int r = gr + j;
            if (r < Kout) {
              int cij = imod<POW2>(r, cs.d_cin);
              int kj = idiv<POW2>(r, cs.d_cin);
              int kwj = kj % cs.KW, khj = kj / cs.KW;
              int ih = oh * cs.SH - cs.PH + khj;
              int iw = ow * cs.SW - cs.PW + kwj;
              if (ih >= 0 && ih < cs.H && iw >= 0 && iw < cs.W)
                v.e[j] = X[(((int64_t)n * cs.H + ih) * cs.W + iw) * cs.Cin + cij];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        As[lds_off<T>(rr + j, mm)] = v.e[j];
    }
    // ---- stage B: dy[m][co] -> Bs[co][m] ----
#pragma unroll
    for (int c = threadIdx.x; c < BK * (BN / V); c += THREADS) {
      int mm = c / (BN / V);
      int nn = (c % (BN / V)) * V;
      int gm = k0 + mm;
      int gn = n0 + nn;
      VecT v = {};
      if (gm < m_end) {
        const T* src = &DY[(int64_t)gm * cs.Cout + gn];
        if (gn + V <= cs.Cout && aligned16(src)) {
          v = *(const VecT*)src;
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (gn + j < cs.Cout) v.e[j] = DY[(int64_t)gm * cs.Cout + gn + j];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        Bs[lds_off<T>(nn + j, mm)] = v.e[j];
    }
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    if (colsum) bsum += colsum_tile_partial(Bs);
    __syncthreads();
  }

  float* out = DW + (int64_t)blockIdx.z * (Kout + bias_row) * cs.Cout;
  epilogue_visit(wc, acc, r0, n0, [&](int row, int col, float v) {
    if (row < Kout && col < cs.Cout) out[(int64_t)row * cs.Cout + col] = v;
  });
  if (colsum) {
    bsum = colsum_tile_finish(bsum);
    int col = n0 + (threadIdx.x >> 2);
    if ((threadIdx.x & 3) == 0 && col < cs.Cout)
      out[(int64_t)Kout * cs.Cout + col] = bsum;
  }
}

// ---------------------------------------------------------------------------
// vector-guaranteed wgrad (Cin%V==0, Cout%V==0, 16B-aligned tensors): stages
// in three phases -- addresses (zero-page for OOB/padding), then all 16B
// loads, then the LDS scatter -- so RA+RB global loads stay in flight.
// The generic kernel's `#pragma unroll 1` staging (needed there to avoid
// 221-256 VGPR spills from per-iteration gather state) serializes to one
// load in flight per wave; holding only pointers between phases keeps the
// live state at ~24 VGPR.
// ---------------------------------------------------------------------------
template <typename T, bool POW2>
__launch_bounds__(THREADS, 3)
__global__ void k_conv_wgrad_vec(const T* __restrict__ X,
                                 const T* __restrict__ DY,
                                 float* __restrict__ DW,
                                 const T* __restrict__ zero16, ConvShape cs,
                                 int bias_row) {
  constexpr int V = 16 / sizeof(T);
  constexpr int RA = BK * (BM / V) / THREADS;
  constexpr int RB = BK * (BN / V) / THREADS;
  __shared__ alignas(16) T As[BM * BK];  // rows = (kh,kw,ci), k = m
  __shared__ alignas(16) T Bs[BN * BK];  // rows = co, k = m
  const int M = cs.N * cs.OH * cs.OW;
  const int Kout = cs.KH * cs.KW * cs.Cin;
  int tr_, tn_;
  // same grouped ordering: the gathered-x A operand [Kout, M] is
  // re-read gridDim.y times without it
  if ((int64_t)(cs.KH * cs.KW * cs.Cin) * cs.N * cs.OH * cs.OW >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tr_, tn_);
  else {
    tr_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int r0 = tr_ * BM;
  const int n0 = tn_ * BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  const bool colsum = bias_row && tr_ == 0;  // see k_conv_wgrad
  float bsum = 0.0f;
  using VecT = Pack16<T>;

  // bf16: each thread owns one 8-row group x 4 consecutive m columns --
  // after the loads an in-thread 8x4 transpose packs 4 m-values per row
  // into one 8B ds_write_b64 (vs 8x ds_write_b16 per load; LDS
  // instruction issue was wgrad's post-phase-separation bottleneck:
  // 48 b16 writes vs 16 MFMAs per thread-chunk). The XOR swizzle flips
  // byte bits 4-6 only, so the 8B alignment survives. fp32 keeps the
  // generic scatter.
  //
  // Software-pipelined (T14 rotate): tile t's registers are written to
  // LDS, then tile t+1's loads are ISSUED into the same (now dead)
  // registers before tile t's MFMA phase — the gather latency lands
  // under the MFMAs instead of being exposed at the head of every
  // chunk (the attention kernels' TStage split, applied here).
  constexpr bool TR = sizeof(T) == 2;
  // lane mapping: consecutive lanes share the m-quad and span the row
  // groups: the 16 lanes' 16B global loads form one contiguous 256B run
  // (the conflict-free same-row/mm-strided write mapping was tried and
  // lost more to broken global coalescing than its bank relief won)
  const int a_rr = TR ? (threadIdx.x & (BM / V - 1)) * V : 0;
  const int a_mm0 = TR ? (threadIdx.x / (BM / V)) * 4 : 0;
  VecT va[RA], vb[RB];
  auto load_tile = [&](int k0) {
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
      const T* p = zero16;
      if (gm < m_end && gr < Kout) {
        int n = idiv<POW2>(gm, cs.d_ohow);
        int rem = gm - n * (cs.OH * cs.OW);
        int oh = idiv<POW2>(rem, cs.d_ow), ow = rem - oh * cs.OW;
        int ci = imod<POW2>(gr, cs.d_cin);
        int kidx = idiv<POW2>(gr, cs.d_cin);
        int kh, kw;
        kdecode(kidx, cs, kh, kw);
        int ih = oh * cs.SH - cs.PH + kh;
        int iw = ow * cs.SW - cs.PW + kw;
        if (ih >= 0 && ih < cs.H && iw >= 0 && iw < cs.W)
          p = &X[(((int64_t)n * cs.H + ih) * cs.W + iw) * cs.Cin + ci];
      }
      asrc[it] = p;
    }
    const T* bsrc[RB];
#pragma unroll
    for (int it = 0; it < RB; ++it) {
      int c = threadIdx.x + it * THREADS;
      int mm = c / (BN / V);
      int nn = (c % (BN / V)) * V;
      int gm = k0 + mm;
      bsrc[it] = (gm < m_end && n0 + nn + V <= cs.Cout)
                     ? &DY[(int64_t)gm * cs.Cout + n0 + nn]
                     : zero16;
    }
#pragma unroll
    for (int it = 0; it < RA; ++it) va[it] = *(const VecT*)asrc[it];
#pragma unroll
    for (int it = 0; it < RB; ++it) vb[it] = *(const VecT*)bsrc[it];
  };

  load_tile(m_begin);
  for (int k0 = m_begin; k0 < m_end; k0 += BK) {
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
    if (k0 + BK < m_end) load_tile(k0 + BK);
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    if (colsum) bsum += colsum_tile_partial(Bs);
    __syncthreads();
  }

  float* out = DW + (int64_t)blockIdx.z * (Kout + bias_row) * cs.Cout;
  epilogue_visit(wc, acc, r0, n0, [&](int row, int col, float v) {
    if (row < Kout && col < cs.Cout) out[(int64_t)row * cs.Cout + col] = v;
  });
  if (colsum) {
    bsum = colsum_tile_finish(bsum);
    int col = n0 + (threadIdx.x >> 2);
    if ((threadIdx.x & 3) == 0 && col < cs.Cout)
      out[(int64_t)Kout * cs.Cout + col] = bsum;
  }
}

// ---------------------------------------------------------------------------
// bf16 wgrad staged the way fwd/dgrad are: pure LDS-DMA, no staging VGPRs,
// no LDS write instructions. Neither operand needs a transpose in memory --
// dy is a row-major [m][Cout] tile and gathered x is [m][(kh,kw,ci)] with
// 16-byte ci runs -- so both images are stored as they lie, m(=k)-major
// (A [BK][BM], B [BK][BN]), and the MFMA fragments are read transposed
// (tile_gemm.h, kmaj_off / tr_frag_issue). A lane's slot in each of its DMA
// instructions never moves, so its (kh,kw,ci) decode is hoisted out of the
// k-loop; per chunk only the (n,oh,ow) decode of its m-rows remains.
// Same gate as k_conv_wgrad_vec<bf16>: all-pow2 shape, Cin%8 == Cout%8 == 0,
// 16B-aligned tensors. Double-buffered k-loop (48 KB LDS, 3 blocks/CU): it
// measured 3-5% ahead of the single-buffer form (24 KB) on the WRN shapes.
// ---------------------------------------------------------------------------
__launch_bounds__(THREADS, 2)  // <=256 regs: MFMA accumulators stay in VGPRs
__global__ void k_conv_wgrad_tr(const bf16* __restrict__ X,
                                const bf16* __restrict__ DY,
                                float* __restrict__ DW,
                                const bf16* __restrict__ zero16, ConvShape cs,
                                int bias_row) {
  constexpr int NA = glds_kmajor_count<BM / 8>();   // A glds per wave (4)
  constexpr int NPER = NA + glds_kmajor_count<BN / 8>();
  // one LDS object per buffer, named statically in the 2x-unrolled k-loop
  __shared__ alignas(16) bf16 As0[BK * BM], As1[BK * BM];  // [m][(kh,kw,ci)]
  __shared__ alignas(16) bf16 Bs0[BK * BN], Bs1[BK * BN];  // [m][co]
  const int M = cs.N * cs.OH * cs.OW;
  const int Kout = cs.KH * cs.KW * cs.Cin;
  int tr_, tn_;
  if ((int64_t)Kout * M > (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tr_, tn_);
  else {
    tr_ = blockIdx.x;
    tn_ = blockIdx.y;
  }
  const int r0 = tr_ * BM;
  const int n0 = tn_ * BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  const int wm = wc.wid / WAVES_N;
  f32x4 acc[FM][FN] = {};
  // bias gradient (see k_conv_wgrad): the dy fragments are already in
  // registers, so tile-row 0 sums them with one all-ones MFMA per k-step;
  // wave (wm, wn) takes the 16 columns wcol0 + 16*wm
  const bool colsum = bias_row && tr_ == 0;
  f32x4 bacc = {};
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

  // hoisted A-side column decode, one per glds instruction of this lane
  int a_dh[NA], a_dw[NA], a_ci[NA];  // kh-PH, kw-PW, ci (-1: past Kout)
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int row = 4 * (wc.wid * NA + i) + wc.lane / 16;
    const int gr = r0 + 8 * ((wc.lane % 16) ^ kmaj_key<16>(row));
    int kh, kw;
    kdecode(gr >> cs.d_cin.lg, cs, kh, kw);
    a_dh[i] = kh - cs.PH;
    a_dw[i] = kw - cs.PW;
    a_ci[i] = gr < Kout ? (gr & (cs.Cin - 1)) : -1;
  }

  auto stage = [&](int k0, bf16* a_img, bf16* b_img) {
    glds_stage_kmajor<BM / 8>(a_img, wc,
                              [&](int i, int row, int) -> const bf16* {
      // branch-free: an invalid lane's address is computed but never used
      const int gm = k0 + row;
      const int n = gm >> cs.d_ohow.lg;
      const int rem = gm & (cs.OH * cs.OW - 1);
      const int oh = rem >> cs.d_ow.lg, ow = rem & (cs.OW - 1);
      const int ih = oh * cs.SH + a_dh[i];
      const int iw = ow * cs.SW + a_dw[i];
      const bool ok = gm < m_end && a_ci[i] >= 0 &&
                      (unsigned)ih < (unsigned)cs.H &&
                      (unsigned)iw < (unsigned)cs.W;
      // all-pow2 gate: the pixel index and the *Cin are shifts
      const int pix = (n << cs.d_hw.lg) + (ih << cs.d_w.lg) + iw;
      const bf16* p = X + (((int64_t)pix << cs.d_cin.lg) + a_ci[i]);
      return ok ? p : zero16;
    });
    glds_stage_kmajor<BN / 8>(b_img, wc,
                              [&](int, int row, int ch) -> const bf16* {
      const int gm = k0 + row, gn = n0 + 8 * ch;
      const bf16* p = DY + (((int64_t)gm << cs.d_cout.lg) + gn);
      return gm < m_end && gn < cs.Cout ? p : zero16;
    });
  };
  auto compute = [&](const bf16* a_img, const bf16* b_img) {
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      TrFrag a[FM], b[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
        a[fm] = tr_frag_issue<BM / 8>(a_img, ks * 32, wc.wrow0 + fm * 16,
                                      wc.lane);
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        b[fn] = tr_frag_issue<BN / 8>(b_img, ks * 32, wc.wcol0 + fn * 16,
                                      wc.lane);
      tr_frags_wait(a, b);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[fm].get(), b[fn].get(), acc[fm][fn], 0, 0, 0);
      if (colsum)
        bacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ones, wm ? b[1].get() : b[0].get(), bacc, 0, 0, 0);
    }
  };

  // chunk k0 sits in (a_cur, b_cur); the next one streams into the other
  // buffer under this chunk's MFMAs
  auto step = [&](int k0, bf16* a_cur, bf16* b_cur, bf16* a_nxt,
                  bf16* b_nxt) {
    if (k0 + BK < m_end) {
      stage(k0 + BK, a_nxt, b_nxt);
      wait_vmcnt<NPER>();   // this chunk landed; the next stays in flight
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    compute(a_cur, b_cur);
    __builtin_amdgcn_s_barrier();   // cur free for the chunk after next
  };
  if (m_begin < m_end) stage(m_begin, As0, Bs0);
  for (int k0 = m_begin; k0 < m_end; k0 += 2 * BK) {
    step(k0, As0, Bs0, As1, Bs1);
    if (k0 + BK < m_end) step(k0 + BK, As1, Bs1, As0, Bs0);
  }

  float* out = DW + (int64_t)blockIdx.z * (Kout + bias_row) * cs.Cout;
  epilogue_visit(wc, acc, r0, n0, [&](int row, int col, float v) {
    if (row < Kout && col < cs.Cout) out[(int64_t)row * cs.Cout + col] = v;
  });
  if (colsum && wc.lane < 16) {
    // every row of bacc is the column sum; lanes 0-15 hold row 0
    int col = n0 + wc.wcol0 + 16 * wm + wc.lane;
    if (col < cs.Cout) out[(int64_t)Kout * cs.Cout + col] = bacc[0];
  }
}

// ---------------------------------------------------------------------------
// batched LDS-tiled 2D transpose: out[b][c][r] = in[b][r][c]. 32x32 tiles,
// coalesced on both sides (the naive elementwise form writes strided and
// measured 2.6 TB/s; this hits ~5).
template <typename T>
__global__ void k_transpose2d_tiled(const T* __restrict__ in,
                                    T* __restrict__ out, int rows, int cols) {
  __shared__ T tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int64_t slice = (int64_t)blockIdx.z * rows * cols;
  const T* src = in + slice;
  T* dst = out + slice;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32x8
#pragma unroll
  for (int d = 0; d < 32; d += 8) {
    int r = r0 + ty + d, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + d][tx] = src[(int64_t)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < 32; d += 8) {
    int c = c0 + ty + d, r = r0 + tx;
    if (c < cols && r < rows) dst[(int64_t)c * rows + r] = tile[tx][ty + d];
  }
}

// ---------------------------------------------------------------------------
// [KH,KW,Ci,Co] -> [Ci, KH*KW*Co] (k-contiguous rows for the dgrad B glds)
template <typename T>
__global__ void k_transpose_w_dgrad(const T* __restrict__ W,
                                    T* __restrict__ WT2D, int KHW, int Cin,
                                    int Cout) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t n = (int64_t)KHW * Cin * Cout;
  if (i >= n) return;
  int co = i % Cout;
  int ci = (i / Cout) % Cin;
  int64_t khw = i / ((int64_t)Cin * Cout);
  WT2D[((int64_t)ci * KHW + khw) * Cout + co] = W[i];
}

// co stays the inner dim on both sides: move whole 16B chunks, coalesced
// reads AND writes
template <typename T>
__global__ void k_transpose_w_dgrad_vec(const T* __restrict__ W,
                                        T* __restrict__ WT2D, int KHW,
                                        int Cin, int Cout) {
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) P { T e[16 / sizeof(T)]; };
  const int cov = Cout / V;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t n = (int64_t)KHW * Cin * cov;
  if (i >= n) return;
  int c = i % cov;
  int ci = (i / cov) % Cin;
  int64_t khw = i / ((int64_t)Cin * cov);
  ((P*)WT2D)[((int64_t)ci * KHW + khw) * cov + c] =
      ((const P*)W)[((int64_t)khw * Cin + ci) * cov + c];
}

// ---------------------------------------------------------------------------
static bool all_pow2(const ConvShape& cs) {
  return cs.d_ohow.lg >= 0 && cs.d_ow.lg >= 0 && cs.d_cin.lg >= 0 &&
         cs.d_hw.lg >= 0 && cs.d_w.lg >= 0 && cs.d_cout.lg >= 0;
}

// k-loop length up to which the double buffer is used (TNN_DB_MAXK, read
// once). Past it bf16 takes the single-buffer form of the same DMA-staged
// tile; fp32 falls back to k_conv_fwd.
static int fwd_db_maxk() {
  static const int maxk = []() {
    const char* e = getenv("TNN_DB_MAXK");
    return e ? atoi(e) : 2304;
  }();
  return maxk;
}

// true: the launcher wants the [Cout][K] weight and takes a DMA-staged
// kernel, which also carries the fused statistics epilogue
bool conv2d_fwd_wants_db(DT dt, const void* x, const ConvShape& cs) {
  static const bool db_on = []() {
    const char* e = getenv("TNN_FWD_DB");
    return !(e && atoi(e) == 0);
  }();
  if (!db_on) return false;
  int v = dt == DT::F32 ? 4 : 8;
  if (dt == DT::F32 && cs.KH * cs.KW * cs.Cin > fwd_db_maxk()) return false;
  return all_pow2(cs) && cs.Cin % v == 0 && (((uintptr_t)x & 15) == 0);
}

void transpose_w_fwd_launch(DT dt, const void* w, void* w_t2, int KHW, int Cin,
                            int Cout, hipStream_t s) {
  // [KHW*Cin, Cout] -> [Cout, KHW*Cin] is a plain 2D transpose
  int rows = KHW * Cin;
  dim3 grid((Cout + 31) / 32, (rows + 31) / 32, 1);
  if (dt == DT::F32)
    hipLaunchKernelGGL(k_transpose2d_tiled<float>, grid, dim3(256), 0, s,
                       (const float*)w, (float*)w_t2, rows, Cout);
  else
    hipLaunchKernelGGL(k_transpose2d_tiled<bf16>, grid, dim3(256), 0, s,
                       (const bf16*)w, (bf16*)w_t2, rows, Cout);
}

void conv2d_fwd_launch(DT dt, const void* x, const void* w, const void* w_t2,
                       const void* bias, void* y, const void* zero16,
                       float* stats, const ConvShape& cs, bool relu,
                       hipStream_t s) {
  int M = cs.N * cs.OH * cs.OW;
  dim3 grid(ceil_div(M, BM), ceil_div(cs.Cout, BN));
  int act = relu ? ACT_RELU : ACT_LINEAR;
  bool p2 = all_pow2(cs);
  if (dt == DT::F32) {
    if (w_t2) {
      auto kern = stats ? k_conv_fwd_db<float, true, true>
                        : k_conv_fwd_db<float, true>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const float*)x,
                         (const float*)w_t2, (const float*)bias,
                         (const float*)nullptr, (float*)y,
                         (const float*)zero16, cs, act, stats);
      return;
    }
    bool g = p2 && cs.Cin % 4 == 0 && (((uintptr_t)x & 15) == 0);
    auto kern = g ? k_conv_fwd<float, true, true>
                  : (p2 ? k_conv_fwd<float, true, false>
                        : k_conv_fwd<float, false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s,
                       (const float*)x, (const float*)w, (const float*)bias,
                       (const float*)nullptr, (float*)y, (const float*)zero16,
                       cs, act);
  } else {
    if (w_t2 && cs.KH * cs.KW * cs.Cin > fwd_db_maxk()) {
      auto kern = stats ? k_conv_fwd_sb<true> : k_conv_fwd_sb<false>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const bf16*)x,
                         (const bf16*)w_t2, (const bf16*)bias, (bf16*)y,
                         (const bf16*)zero16, cs, act, stats);
      return;
    }
    if (w_t2) {
      auto kern = stats ? k_conv_fwd_db<bf16, true, true>
                        : k_conv_fwd_db<bf16, true>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const bf16*)x,
                         (const bf16*)w_t2, (const float*)nullptr,
                         (const bf16*)bias, (bf16*)y, (const bf16*)zero16, cs,
                         act, stats);
      return;
    }
    bool g = p2 && cs.Cin % 8 == 0 && (((uintptr_t)x & 15) == 0);
    auto kern = g ? k_conv_fwd<bf16, true, true>
                  : (p2 ? k_conv_fwd<bf16, true, false>
                        : k_conv_fwd<bf16, false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s,
                       (const bf16*)x, (const bf16*)w, (const float*)nullptr,
                       (const bf16*)bias, (bf16*)y, (const bf16*)zero16, cs,
                       act);
  }
}

bool conv2d_dgrad_wants_db(DT dt, const void* dy, const ConvShape& cs) {
  static const bool db_on = []() {
    const char* e = getenv("TNN_FWD_DB");
    return !(e && atoi(e) == 0);
  }();
  if (!db_on) return false;
  static const int maxk = []() {
    const char* e = getenv("TNN_DB_MAXK_DGRAD");
    return e ? atoi(e) : 4608;  // dgrad ties-or-wins with DB up to here
  }();
  int v = dt == DT::F32 ? 4 : 8;
  return cs.KH * cs.KW * cs.Cout <= maxk && all_pow2(cs) &&
         cs.Cout % v == 0 && (((uintptr_t)dy & 15) == 0);
}

void transpose_w_dgrad_launch(DT dt, const void* w, void* w_t2d, int KHW,
                              int Cin, int Cout, hipStream_t s) {
  int V = dt == DT::F32 ? 4 : 8;
  if (Cout % V == 0 && (((uintptr_t)w & 15) == 0)) {
    int64_t n = (int64_t)KHW * Cin * (Cout / V);
    int blocks = (int)((n + 255) / 256);
    if (dt == DT::F32)
      hipLaunchKernelGGL(k_transpose_w_dgrad_vec<float>, dim3(blocks),
                         dim3(256), 0, s, (const float*)w, (float*)w_t2d, KHW,
                         Cin, Cout);
    else
      hipLaunchKernelGGL(k_transpose_w_dgrad_vec<bf16>, dim3(blocks),
                         dim3(256), 0, s, (const bf16*)w, (bf16*)w_t2d, KHW,
                         Cin, Cout);
    return;
  }
  int64_t n = (int64_t)KHW * Cin * Cout;
  int blocks = (int)((n + 255) / 256);
  if (dt == DT::F32)
    hipLaunchKernelGGL(k_transpose_w_dgrad<float>, dim3(blocks), dim3(256), 0,
                       s, (const float*)w, (float*)w_t2d, KHW, Cin, Cout);
  else
    hipLaunchKernelGGL(k_transpose_w_dgrad<bf16>, dim3(blocks), dim3(256), 0,
                       s, (const bf16*)w, (bf16*)w_t2d, KHW, Cin, Cout);
}

void conv2d_dgrad_launch(DT dt, const void* dy, const void* w_t,
                         const void* w_t2d, void* dx, const void* zero16,
                         const ConvShape& cs, hipStream_t s) {
  int M = cs.N * cs.H * cs.W;
  dim3 grid(ceil_div(M, BM), ceil_div(cs.Cin, BN));
  bool p2 = all_pow2(cs);
  // stride-2 parity decomposition (see k_conv_dgrad<..., S2>): 4 classes in
  // grid.z over an M/4-row problem with only the stride-compatible (kh,kw)
  // taps in K. Requires even spatial dims; routed through the glds variant.
  bool s2 = p2 && cs.SH == 2 && cs.SW == 2 && cs.H % 2 == 0 && cs.W % 2 == 0;
  ConvShape cs2 = cs;
  if (s2) {
    cs2.d_hw.set((cs.H / 2) * (cs.W / 2));
    cs2.d_w.set(cs.W / 2);
    s2 = cs2.d_hw.lg >= 0 && cs2.d_w.lg >= 0;
  }
  dim3 grid_s2(ceil_div(cs.N * (cs.H / 2) * (cs.W / 2), BM),
               ceil_div(cs.Cin, BN), 4);
  if (dt == DT::F32) {
    bool g = p2 && cs.Cout % 4 == 0 && (((uintptr_t)dy & 15) == 0);
    if (w_t2d && s2) {
      hipLaunchKernelGGL((k_conv_dgrad_db<float, true, true>), grid_s2,
                         dim3(THREADS), 0, s, (const float*)dy,
                         (const float*)w_t2d, (float*)dx, (const float*)zero16,
                         cs2);
      return;
    }
    if (w_t2d) {
      auto kern = cs.SH == 1 && cs.SW == 1
                      ? k_conv_dgrad_db<float, true, false, true>
                      : k_conv_dgrad_db<float, true>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const float*)dy,
                         (const float*)w_t2d, (float*)dx,
                         (const float*)zero16, cs);
      return;
    }
    if (g && s2) {
      hipLaunchKernelGGL((k_conv_dgrad<float, true, true, true>), grid_s2,
                         dim3(THREADS), 0, s, (const float*)dy,
                         (const float*)w_t, (float*)dx, (const float*)zero16,
                         cs2);
      return;
    }
    bool s1 = cs.SH == 1 && cs.SW == 1;
    auto kern = g ? (s1 ? k_conv_dgrad<float, true, true, false, true>
                        : k_conv_dgrad<float, true, true>)
                  : (p2 ? k_conv_dgrad<float, true, false>
                        : k_conv_dgrad<float, false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s,
                       (const float*)dy, (const float*)w_t, (float*)dx,
                       (const float*)zero16, cs);
  } else {
    bool g = p2 && cs.Cout % 8 == 0 && (((uintptr_t)dy & 15) == 0);
    if (w_t2d && s2) {
      hipLaunchKernelGGL((k_conv_dgrad_db<bf16, true, true>), grid_s2,
                         dim3(THREADS), 0, s, (const bf16*)dy,
                         (const bf16*)w_t2d, (bf16*)dx, (const bf16*)zero16,
                         cs2);
      return;
    }
    if (w_t2d) {
      auto kern = cs.SH == 1 && cs.SW == 1
                      ? k_conv_dgrad_db<bf16, true, false, true>
                      : k_conv_dgrad_db<bf16, true>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const bf16*)dy,
                         (const bf16*)w_t2d, (bf16*)dx, (const bf16*)zero16,
                         cs);
      return;
    }
    if (g && s2) {
      hipLaunchKernelGGL((k_conv_dgrad<bf16, true, true, true>), grid_s2,
                         dim3(THREADS), 0, s, (const bf16*)dy,
                         (const bf16*)w_t, (bf16*)dx, (const bf16*)zero16,
                         cs2);
      return;
    }
    bool s1 = cs.SH == 1 && cs.SW == 1;
    auto kern = g ? (s1 ? k_conv_dgrad<bf16, true, true, false, true>
                        : k_conv_dgrad<bf16, true, true>)
                  : (p2 ? k_conv_dgrad<bf16, true, false>
                        : k_conv_dgrad<bf16, false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s,
                       (const bf16*)dy, (const bf16*)w_t, (bf16*)dx,
                       (const bf16*)zero16, cs);
  }
}

int conv2d_wgrad_zsplits(const ConvShape& cs) {
  int M = cs.N * cs.OH * cs.OW;
  int Kout = cs.KH * cs.KW * cs.Cin;
  int base = ceil_div(Kout, BM) * ceil_div(cs.Cout, BN);
  int want = 2048;
  int z = base >= want ? 1
                       : std::min(ceil_div(M, 4 * BK), ceil_div(want, base));
  return std::max(z, 1);
}

void conv2d_wgrad_launch(DT dt, const void* x, const void* dy, void* dw_out,
                         DT out_dt, float* ws, int z, const void* zero16,
                         const ConvShape& cs, bool bias, hipStream_t s) {
  int Kout = cs.KH * cs.KW * cs.Cin;
  // bias: dw_out and every slab carry one more row, [Kout+1][Cout], whose
  // last row is the bias gradient sum_m dy (summed by the tile-row-0 blocks)
  const int bias_row = bias ? 1 : 0;
  // bf16 output always goes through the (casting) reduce; fp32 with z==1
  // writes the slab target directly
  bool direct = z == 1 && out_dt == DT::F32;
  float* target = direct ? (float*)dw_out : ws;
  dim3 grid(ceil_div(Kout, BM), ceil_div(cs.Cout, BN), z);
  bool p2 = all_pow2(cs);
  if (dt == DT::F32) {
    bool vec = p2 && cs.Cin % 4 == 0 && cs.Cout % 4 == 0 &&
               (((uintptr_t)x & 15) == 0) && (((uintptr_t)dy & 15) == 0);
    if (vec) {
      hipLaunchKernelGGL((k_conv_wgrad_vec<float, true>), grid, dim3(THREADS),
                         0, s, (const float*)x, (const float*)dy, target,
                         (const float*)zero16, cs, bias_row);
    } else {
      auto kern = p2 ? k_conv_wgrad<float, true> : k_conv_wgrad<float, false>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const float*)x,
                         (const float*)dy, target, cs, bias_row);
    }
  } else {
    bool vec = p2 && cs.Cin % 8 == 0 && cs.Cout % 8 == 0 &&
               (((uintptr_t)x & 15) == 0) && (((uintptr_t)dy & 15) == 0);
    // TNN_WGRAD_TR=0 (read once) routes bf16 back to the register-staged
    // kernel, so both paths can be compared from one build
    static const bool tr_on = []() {
      const char* e = getenv("TNN_WGRAD_TR");
      return !(e && atoi(e) == 0);
    }();
    if (vec && tr_on) {
      hipLaunchKernelGGL(k_conv_wgrad_tr, grid, dim3(THREADS), 0, s,
                         (const bf16*)x,
                         (const bf16*)dy, target, (const bf16*)zero16, cs,
                         bias_row);
    } else if (vec) {
      hipLaunchKernelGGL((k_conv_wgrad_vec<bf16, true>), grid, dim3(THREADS),
                         0, s, (const bf16*)x, (const bf16*)dy, target,
                         (const bf16*)zero16, cs, bias_row);
    } else {
      auto kern = p2 ? k_conv_wgrad<bf16, true> : k_conv_wgrad<bf16, false>;
      hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, (const bf16*)x,
                         (const bf16*)dy, target, cs, bias_row);
    }
  }
  // the reduce kernel (and so dw's summation order) is chosen from dw's own
  // size: with Cout % 4 == 0 the extra row never changes dw's bits (else the
  // longer output can fall off the float4 reduce; still deterministic)
  if (!direct)
    splitk_reduce_launch(ws, dw_out, out_dt, z,
                         (int64_t)(Kout + bias_row) * cs.Cout, s,
                         (int64_t)Kout * cs.Cout);
}

void transpose_w_launch(DT dt, const void* w, void* w_t, int KH, int KW,
                        int Cin, int Cout, hipStream_t s) {
  // batched [Cin, Cout] -> [Cout, Cin] transpose per (kh,kw) slice
  dim3 grid((Cout + 31) / 32, (Cin + 31) / 32, KH * KW);
  if (dt == DT::F32)
    hipLaunchKernelGGL(k_transpose2d_tiled<float>, grid, dim3(256), 0, s,
                       (const float*)w, (float*)w_t, Cin, Cout);
  else
    hipLaunchKernelGGL(k_transpose2d_tiled<bf16>, grid, dim3(256), 0, s,
                       (const bf16*)w, (bf16*)w_t, Cin, Cout);
}

}  // namespace tnn
