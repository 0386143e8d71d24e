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
// pieces shared by the kernel bodies below
// ---------------------------------------------------------------------------

// this block's (tm, tn) tile: grouped tile order once the gathered activation
// stream (im2col elements) exceeds the 256 MiB L3 across its n-tile re-reads
// (see tile_gemm.h), dispatch order below that
DEV void conv_tile_order(const ConvShape& cs, int& tm, int& tn) {
  if ((int64_t)cs.N * cs.OH * cs.OW * (cs.KH * cs.KW * cs.Cin) >
      (int64_t)32 * 1024 * 1024)
    tile::tile_remap_xcd<4>(tm, tn);
  else {
    tm = blockIdx.x;
    tn = blockIdx.y;
  }
}

// ---- forward gather: im2col element (gm, gk) of x --------------------------
// row gm = (n, oh, ow), held as the image and the input pixel of tap (0, 0)
struct FwdRow { int n, ih0, iw0; };
template <bool POW2>
DEV FwdRow fwd_row(const ConvShape& cs, int gm) {
  int n = idiv<POW2>(gm, cs.d_ohow);
  int rem = gm - n * (cs.OH * cs.OW);
  int oh = idiv<POW2>(rem, cs.d_ow), ow = rem - oh * cs.OW;
  return {n, oh * cs.SH - cs.PH, ow * cs.SW - cs.PW};
}
// address of x at k index gk = (kh, kw, ci), or oob (null, the zero page)
// when the tap falls into the padding
template <bool POW2, typename T>
DEV const T* fwd_src(const T* __restrict__ X, const ConvShape& cs,
                     const FwdRow& r, int gk, const T* oob) {
  int ci = imod<POW2>(gk, cs.d_cin);
  int kidx = idiv<POW2>(gk, cs.d_cin);
  int kh, kw;
  kdecode(kidx, cs, kh, kw);
  int ih = r.ih0 + kh;
  int iw = r.iw0 + kw;
  if (ih < 0 || ih >= cs.H || iw < 0 || iw >= cs.W) return oob;
  return &X[(((int64_t)r.n * cs.H + ih) * cs.W + iw) * cs.Cin + ci];
}
// 16 bytes of row r at k indices [gk, gk + V), zero in the padding and at or
// past K: one vector load when the run lies in one (kh,kw) slice, else
// element-wise
template <bool POW2, typename T>
DEV Pack16<T> fwd_gather16(const T* __restrict__ X, const ConvShape& cs,
                           const FwdRow& r, int gk, int K) {
  constexpr int V = 16 / sizeof(T);
  Pack16<T> v = {};
  const T* const none = nullptr;
  if (imod<POW2>(gk, cs.d_cin) + V <= cs.Cin && gk + V <= K &&
      (cs.Cin % V) == 0 && aligned16(X)) {
    if (const T* p = fwd_src<POW2>(X, cs, r, gk, none))
      v = *(const Pack16<T>*)p;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (gk + j >= K) continue;
      if (const T* p = fwd_src<POW2>(X, cs, r, gk + j, none)) v.e[j] = *p;
    }
  }
  return v;
}

// ---- dgrad gather: dy element behind dx pixel (n, ih, iw) and tap (kh, kw) --
// S2: stride-2 parity decomposition. blockIdx.z selects the (ih%2, iw%2) class
// so every (kh,kw) visited satisfies the stride divisibility test by
// construction -- the generic kernel at stride 2 burns 3/4 of its MFMAs
// multiplying gathered zeros. A class is an M/4-row problem over the
// compacted taps (khi, kwi) -> (start_h + 2 khi, start_w + 2 kwi); the
// launcher rewrites cs.d_hw/d_w to the per-class (Hc*Wc, Wc) divisors.
// Without S2 the one "class" is the whole problem.
struct DgradTap { int khi, kwi, kh, kw, widx; };  // widx: tap index kh*KW+kw
template <bool S2>
struct DgradClass {
  int cls_a, cls_b, start_h, start_w, nkh, nkw, Hc, Wc, M, K;
  DEV explicit DgradClass(const ConvShape& cs) {
    cls_a = S2 ? ((int)blockIdx.z >> 1) : 0;
    cls_b = S2 ? ((int)blockIdx.z & 1) : 0;
    start_h = S2 ? ((cls_a + cs.PH) & 1) : 0;
    start_w = S2 ? ((cls_b + cs.PW) & 1) : 0;
    nkh = S2 ? ((cs.KH - start_h + 1) >> 1) : cs.KH;
    nkw = S2 ? ((cs.KW - start_w + 1) >> 1) : cs.KW;
    Hc = S2 ? (cs.H >> 1) : cs.H;
    Wc = S2 ? (cs.W >> 1) : cs.W;
    M = cs.N * Hc * Wc;
    K = nkh * nkw * cs.Cout;
  }
  // kidx = k index / Cout of this class -> its tap
  DEV DgradTap tap(const ConvShape& cs, int kidx) const {
    DgradTap t;
    if constexpr (S2) {
      // nkw is 1 or 2: dgrad_parity admits KW <= 4 only (nkw = 3 or 4 would
      // need a real division here); nkh is free, khi takes what is left
      t.kwi = kidx & (nkw - 1);
      t.khi = nkw == 2 ? (kidx >> 1) : kidx;
      t.kh = start_h + 2 * t.khi;
      t.kw = start_w + 2 * t.kwi;
      t.widx = t.kh * cs.KW + start_w + 2 * t.kwi;
    } else {
      kdecode(kidx, cs, t.kh, t.kw);
      t.khi = t.kh;
      t.kwi = t.kw;
      t.widx = kidx;
    }
    return t;
  }
  // class row -> (n, ih, iw) of dx
  template <bool POW2>
  DEV void coords(const ConvShape& cs, int row, int& n, int& ih, int& iw) const {
    n = idiv<POW2>(row, cs.d_hw);
    int rem = row - n * (Hc * Wc);
    ih = idiv<POW2>(rem, cs.d_w);
    iw = rem - ih * Wc;
    if constexpr (S2) {
      ih = 2 * ih + cls_a;
      iw = 2 * iw + cls_b;
    }
  }
  // class row -> pixel index of dx
  template <bool POW2>
  DEV int64_t pixel(const ConvShape& cs, int row) const {
    if constexpr (!S2) return row;
    int n, ih, iw;
    coords<POW2>(cs, row, n, ih, iw);
    return ((int64_t)n * cs.H + ih) * cs.W + iw;
  }
};
// address of dy at (n, oh, ow, co), the output pixel that feeds dx pixel
// (ih, iw) through tap (kh, kw), or oob (null, the zero page) when there is
// none. S2: th, tw are even by construction; S1: oh == th; otherwise the
// stride is tested at run time.
template <bool S2, bool S1, typename T>
DEV const T* dgrad_src(const T* __restrict__ DY, const ConvShape& cs, int n,
                       int ih, int iw, int kh, int kw, int co, const T* oob) {
  int th = ih + cs.PH - kh, tw = iw + cs.PW - kw;
  int oh, ow;
  if constexpr (S2) {
    if (th < 0 || tw < 0) return oob;
    oh = th >> 1, ow = tw >> 1;
    if (oh >= cs.OH || ow >= cs.OW) return oob;
  } else if constexpr (S1) {
    if (th < 0 || tw < 0 || th >= cs.OH || tw >= cs.OW) return oob;
    oh = th, ow = tw;
  } else {
    if (th < 0 || tw < 0 || th % cs.SH || tw % cs.SW) return oob;
    oh = th / cs.SH, ow = tw / cs.SW;
    if (oh >= cs.OH || ow >= cs.OW) return oob;
  }
  return &DY[(((int64_t)n * cs.OH + oh) * cs.OW + ow) * cs.Cout + co];
}

// ---- register-staged operand images ----------------------------------------
// A: the [BM][BK] image of rows m0.. and k indices k0.., gathered 16 bytes at
// a time by gather(gm, gk); rows >= M and k >= K are zero
template <typename T, typename GatherFn>
DEV void stage_a_gathered(T* As, int m0, int k0, int M, int K,
                          GatherFn&& gather) {
  constexpr int V = 16 / sizeof(T);
#pragma unroll
  for (int c = threadIdx.x; c < BM * (BK / V); c += THREADS) {
    int row = c / (BK / V);
    int kk = (c % (BK / V)) * V;
    int gm = m0 + row, gk = k0 + kk;
    Pack16<T> v = {};
    if (gm < M && gk < K) v = gather(gm, gk);
    *(Pack16<T>*)&As[lds_off<T>(row, kk)] = v;
  }
}
// B: rows k0.. of a row-major matrix (rowptr(gk) -> its row, ncols wide),
// columns n0.., scatter-transposed into the image Bs[n][k]; rows >= K and
// columns >= ncols are zero
template <typename T, typename RowFn>
DEV void stage_b_transposed(T* Bs, RowFn&& rowptr, int ncols, int n0, int k0,
                            int K) {
  constexpr int V = 16 / sizeof(T);
#pragma unroll
  for (int c = threadIdx.x; c < BK * (BN / V); c += THREADS) {
    int kk = c / (BN / V);
    int nn = (c % (BN / V)) * V;
    int gk = k0 + kk;
    Pack16<T> v = {};
    if (gk < K) v = load16_guarded(rowptr(gk), n0 + nn, ncols);
#pragma unroll
    for (int j = 0; j < V; ++j)
      Bs[lds_off<T>(nn + j, kk)] = v.e[j];
  }
}

// ---- epilogues --------------------------------------------------------------
// Their pointer parameters carry no __restrict__ of their own: the kernels'
// qualifiers hold after inlining, and repeating them here changed the
// instruction selection of the DMA-staged kernels' epilogues.

// fwd: y = act(acc + bias), cast store
template <typename T, typename S>
DEV void conv_fwd_store(const WaveCoordT<S>& wc, f32x4 acc[S::FM][S::FN],
                        const T* bias, T* Y, const ConvShape& cs, int act_kind,
                        int m0, int n0, int M) {
  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < M && col < cs.Cout) {
      if (bias) v += VecIO<T>::to_f32(bias[col]);
      if (act_kind != ACT_LINEAR) v = act_apply(v, act_kind);
      Y[(int64_t)row * cs.Cout + col] = VecIO<T>::from_f32(v);
    }
  });
}

// fwd fused statistics: per-channel sum/sumsq of the tile straight from the
// accumulators (post-bias, linear act only): saves the BN stats pass's full
// read of y. C/D fragment col = lane&15; lanes {l, l+16, l+32, l+48} share
// a column -> two shfl_xor folds give one partial per (wave, col). The
// WAVES_M waves of the block that share a column fold through a small LDS
// array of its own (2 KB; the k-loop's buffers are not touched), in wave
// order, and the block stores one [2][BN] partial with plain stores into
// partials[tm][2][Cout], tm the m-tile after the tile-order remap. No atomics,
// no zero-init: every (tm, col) is written by exactly one block, and the rows
// are summed by a fold in a fixed order (slab_fin_launch / k_bn_finalize_fold),
// so two calls give the same bits. Every thread of the block must call this.
template <typename T, typename S>
DEV void conv_fwd_stats(const WaveCoordT<S>& wc, f32x4 acc[S::FM][S::FN],
                        const T* bias_p, float* partials, const ConvShape& cs,
                        int tm, int m0, int n0, int M) {
  constexpr int FM = S::FM, FN = S::FN;
  __shared__ float red[2][S::WAVES_M][S::BN];
  const int wm = wc.wid / S::WAVES_N;
  const int cr = (wc.lane >> 4) * 4;
  const int cc = wc.lane & 15;
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int lcol = wc.wcol0 + fn * 16 + cc;
    int col = n0 + lcol;
    float bias = 0.0f;
    if (col < cs.Cout) {
      if (bias_p) bias = VecIO<T>::to_f32(bias_p[col]);
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
    if (wc.lane < 16) {
      red[0][wm][lcol] = s;
      red[1][wm][lcol] = ss;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * S::BN; i += THREADS) {
    const int which = i / S::BN, lcol = i % S::BN;
    const int col = n0 + lcol;
    if (col >= cs.Cout) continue;
    float a = red[which][0][lcol];
#pragma unroll
    for (int w = 1; w < S::WAVES_M; ++w) a += red[which][w][lcol];
    partials[((int64_t)tm * 2 + which) * cs.Cout + col] = a;
  }
}

// dgrad: cast store of a class's rows to their dx pixels
template <bool POW2, typename T, bool S2, typename S>
DEV void dgrad_store(const WaveCoordT<S>& wc, f32x4 acc[S::FM][S::FN], T* DX,
                     const ConvShape& cs, const DgradClass<S2>& dc, int m0,
                     int n0) {
  epilogue_visit(wc, acc, m0, n0, [&](int row, int col, float v) {
    if (row < dc.M && col < cs.Cin)
      DX[dc.template pixel<POW2>(cs, row) * cs.Cin + col] =
          VecIO<T>::from_f32(v);
  });
}

// wgrad: block z's tile into slab z of the [z][Kout + bias_row][Cout] fp32
// workspace; returns the slab
template <typename S>
DEV float* wgrad_slab_store(const WaveCoordT<S>& wc,
                            f32x4 acc[S::FM][S::FN], float* DW,
                            const ConvShape& cs, int Kout, int bias_row,
                            int r0, int n0) {
  float* out = DW + (int64_t)blockIdx.z * (Kout + bias_row) * cs.Cout;
  epilogue_visit(wc, acc, r0, n0, [&](int row, int col, float v) {
    if (row < Kout && col < cs.Cout) out[(int64_t)row * cs.Cout + col] = v;
  });
  return out;
}
// bias gradient of the transposed-read kernels: wave (wm, wn) of a tile-row-0
// block summed fragment columns wcol0 + 16 * (NBF * wm + t) with all-ones
// MFMAs; every row of bacc[t] is the column sum and lanes 0-15 hold row 0
template <typename S>
DEV void wgrad_biasrow_store(float* out, const WaveCoordT<S>& wc,
                             const f32x4 (&bacc)[S::FN / S::WAVES_M],
                             const ConvShape& cs, int Kout, int n0) {
  constexpr int NBF = S::FN / S::WAVES_M;
  const int wm = wc.wid / S::WAVES_N;
  if (wc.lane < 16) {
#pragma unroll
    for (int t = 0; t < NBF; ++t) {
      int col = n0 + wc.wcol0 + 16 * (NBF * wm + t) + wc.lane;
      if (col < cs.Cout) out[(int64_t)Kout * cs.Cout + col] = bacc[t][0];
    }
  }
}
// bias gradient of the register-staged kernels: the per-thread dy column
// partials bsum of a tile-row-0 block, folded into row Kout of its slab
DEV void wgrad_colsum_store(float* out, const ConvShape& cs, int Kout, int n0,
                            float bsum) {
  bsum = colsum_tile_finish(bsum);
  int col = n0 + (threadIdx.x >> 2);
  if ((threadIdx.x & 3) == 0 && col < cs.Cout)
    out[(int64_t)Kout * cs.Cout + col] = bsum;
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
// The tile shape S comes with wc: the images are [S::BM][BK] and [S::BN][BK],
// filled by S::BM/32 + S::BN/32 bf16 DMA instructions per wave and chunk.
template <bool DB, typename T, typename S, typename RowFn, typename TapFn,
          typename AtFn>
DEV void conv_db_kloop(T* As0, T* As1, T* Bs0, T* Bs1,
                       const WaveCoordT<S>& wc, f32x4 acc[S::FM][S::FN],
                       const T* __restrict__ asrc, int lgSW, int lgC,
                       const T* __restrict__ bsrc, int64_t bstride,
                       int brows, int m0, int n0, int K,
                       const T* __restrict__ zero16, RowFn&& row,
                       TapFn&& tap, AtFn&& at) {
  constexpr int NA = glds_count<T, S::BM>();   // A glds per wave
  constexpr int NB = glds_count<T, S::BN>();   // B glds per wave
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
template <typename T, bool STATS, bool DB, typename S = TileStd>
DEV void conv_fwd_glds_tile(const T* __restrict__ X,
                            const T* __restrict__ WT2,
                            const T* __restrict__ bias, T* __restrict__ Y,
                            const T* __restrict__ zero16, const ConvShape& cs,
                            int act_kind, float* __restrict__ stats) {
  const int M = cs.N * cs.OH * cs.OW;
  const int K = cs.KH * cs.KW * cs.Cin;
  int tm_, tn_;
  conv_tile_order(cs, tm_, tn_);
  const int m0 = tm_ * S::BM;
  const int n0 = tn_ * S::BN;
  const WaveCoordT<S> wc;
  f32x4 acc[S::FM][S::FN] = {};

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
    __shared__ alignas(16) T As0[S::BM * BK], As1[S::BM * BK];
    __shared__ alignas(16) T Bs0[S::BN * BK], Bs1[S::BN * BK];
    conv_db_kloop<true>(As0, As1, Bs0, Bs1, wc, acc, X, cs.d_w.lg,
                        cs.d_cin.lg, WT2, (int64_t)K, cs.Cout, m0, n0, K,
                        zero16, row, tap, at);
  } else {
    __shared__ alignas(16) T As0[S::BM * BK], Bs0[S::BN * BK];
    conv_db_kloop<false>(As0, As0, Bs0, Bs0, wc, acc, X, cs.d_w.lg,
                         cs.d_cin.lg, WT2, (int64_t)K, cs.Cout, m0, n0, K,
                         zero16, row, tap, at);
  }

  conv_fwd_store(wc, acc, bias, Y, cs, act_kind, m0, n0, M);
  if constexpr (STATS)
    conv_fwd_stats(wc, acc, bias, stats, cs, tm_, m0, n0, M);
}

template <typename T, bool STATS = false>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd_db(const T* __restrict__ X,
                              const T* __restrict__ WT2,
                              const T* __restrict__ bias, T* __restrict__ Y,
                              const T* __restrict__ zero16, ConvShape cs,
                              int act_kind, float* __restrict__ stats) {
  conv_fwd_glds_tile<T, STATS, true>(X, WT2, bias, Y, zero16, cs, act_kind,
                                     stats);
}

// the same tile on one LDS buffer pair for the long k-loops past the double
// buffer's gate: 24 KB LDS, 72 VGPR + 32 AGPR, register-limited at 4 blocks
// per CU (the double buffer: 3)
template <bool STATS>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd_sb(const bf16* __restrict__ X,
                              const bf16* __restrict__ WT2,
                              const bf16* __restrict__ bias,
                              bf16* __restrict__ Y,
                              const bf16* __restrict__ zero16, ConvShape cs,
                              int act_kind, float* __restrict__ stats) {
  conv_fwd_glds_tile<bf16, STATS, false>(X, WT2, bias, Y, zero16, cs, act_kind,
                                         stats);
}

// the 128x128 tile (TileWide) of the two kernels above, for Cout % 128 == 0:
// 32 KB of images per 2.1 MFLOP chunk where the 128x64 tile stages 24 KB per
// 1.05 MFLOP, and the im2col gather with its address decode is fetched once
// per 128 output channels. Same images, chunk order and MFMA sequence per
// output element, so y is bitwise that of the 128x64 kernels. 64 accumulator
// registers; the double buffer holds 64 KB LDS (2 blocks per CU), the single
// buffer 32 KB and is capped at the 168 registers of 3 waves per SIMD.
template <bool STATS>
__launch_bounds__(THREADS, 2)
__global__ void k_conv_fwd_db_wide(const bf16* __restrict__ X,
                                   const bf16* __restrict__ WT2,
                                   const bf16* __restrict__ bias,
                                   bf16* __restrict__ Y,
                                   const bf16* __restrict__ zero16,
                                   ConvShape cs, int act_kind,
                                   float* __restrict__ stats) {
  conv_fwd_glds_tile<bf16, STATS, true, TileWide>(X, WT2, bias, Y, zero16, cs,
                                                  act_kind, stats);
}
template <bool STATS>
__launch_bounds__(THREADS, 3)
__global__ void k_conv_fwd_sb_wide(const bf16* __restrict__ X,
                                   const bf16* __restrict__ WT2,
                                   const bf16* __restrict__ bias,
                                   bf16* __restrict__ Y,
                                   const bf16* __restrict__ zero16,
                                   ConvShape cs, int act_kind,
                                   float* __restrict__ stats) {
  conv_fwd_glds_tile<bf16, STATS, false, TileWide>(X, WT2, bias, Y, zero16, cs,
                                                   act_kind, stats);
}

// ---------------------------------------------------------------------------
// register-staged forward (GLDS: A by LDS-DMA, which needs the all-pow2
// vector gate; B always through registers, scatter-transposed)
template <typename T, bool POW2, bool GLDS>
__launch_bounds__(THREADS)
__global__ void k_conv_fwd(const T* __restrict__ X, const T* __restrict__ Wt,
                           const T* __restrict__ bias, T* __restrict__ Y,
                           const T* __restrict__ zero16, ConvShape cs,
                           int act_kind) {
  static_assert(!GLDS || POW2, "the LDS-DMA gate implies an all-pow2 shape");
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];

  const int M = cs.N * cs.OH * cs.OW;
  const int K = cs.KH * cs.KW * cs.Cin;
  int tm_, tn_;
  conv_tile_order(cs, tm_, tn_);
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  // fused-im2col source address for a 16B chunk (row, kk elem), or the
  // zero page when the chunk is out of image/padding/tail range; only
  // called on the GLDS path where Cin % V == 0 guarantees one (kh,kw)
  // slice per chunk.
  auto a_src = [&](int k0, int rl, int kk) -> const T* {
    int gm = m0 + rl, gk = k0 + kk;
    if (gm >= M || gk >= K) return zero16;
    return fwd_src<POW2>(X, cs, fwd_row<POW2>(cs, gm), gk, zero16);
  };

  for (int k0 = 0; k0 < K; k0 += BK) {
    if constexpr (GLDS) {
      glds_stage_a<T>(As, wc, [&](int rl, int kk) { return a_src(k0, rl, kk); });
    } else {
      stage_a_gathered(As, m0, k0, M, K, [&](int gm, int gk) {
        return fwd_gather16<POW2>(X, cs, fwd_row<POW2>(cs, gm), gk, K);
      });
    }
    // weights [K, Cout] -> Bs[n][k]
    stage_b_transposed(
        Bs, [&](int gk) { return &Wt[(int64_t)gk * cs.Cout]; }, cs.Cout, n0,
        k0, K);
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }
  conv_fwd_store(wc, acc, bias, Y, cs, act_kind, m0, n0, M);
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
  static_assert(!GLDS || POW2, "the LDS-DMA gate implies an all-pow2 shape");
  static_assert(GLDS || !(S2 || S1), "stride routes are LDS-DMA only");
  constexpr int V = 16 / sizeof(T);
  __shared__ alignas(16) T As[BM * BK];
  __shared__ alignas(16) T Bs[BN * BK];

  const DgradClass<S2> dc(cs);
  const int M = dc.M, K = dc.K;
  int tm_, tn_;
  conv_tile_order(cs, tm_, tn_);
  const int m0 = tm_ * BM;
  const int n0 = tn_ * BN;
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};

  // dy element (gm, gk), gk = (tap, co) of this class; oob in the padding
  // and where the stride does not divide
  auto src = [&](int gm, int gk, const T* oob) {
    int n, ih, iw;
    dc.template coords<POW2>(cs, gm, n, ih, iw);
    int co = imod<POW2>(gk, cs.d_cout);
    const DgradTap t = dc.tap(cs, idiv<POW2>(gk, cs.d_cout));
    return dgrad_src<S2, S1>(DY, cs, n, ih, iw, t.kh, t.kw, co, oob);
  };
  auto a_src = [&](int k0, int rl, int kk) -> const T* {
    int gm = m0 + rl, gk = k0 + kk;
    if (gm >= M || gk >= K) return zero16;
    return src(gm, gk, zero16);
  };

  for (int k0 = 0; k0 < K; k0 += BK) {
    if constexpr (GLDS) {
      glds_stage_a<T>(As, wc, [&](int rl, int kk) { return a_src(k0, rl, kk); });
    } else {
      // gather dy with stride/padding inversion: one vector load when the
      // run lies in one (kh,kw) slice, else element-wise
      stage_a_gathered(As, m0, k0, M, K, [&](int gm, int gk) {
        Pack16<T> v = {};
        if (imod<POW2>(gk, cs.d_cout) + V <= cs.Cout && gk + V <= K &&
            (cs.Cout % V) == 0 && aligned16(DY)) {
          if (const T* p = src(gm, gk, nullptr)) v = *(const Pack16<T>*)p;
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            if (gk + j >= K) continue;
            if (const T* p = src(gm, gk + j, nullptr)) v.e[j] = *p;
          }
        }
        return v;
      });
    }
    // w_t [KH*KW*Cout, Cin] -> Bs[ci][k]; a class's compacted k index maps
    // to the full (kh*KW+kw)*Cout+co row
    stage_b_transposed(
        Bs,
        [&](int gk) {
          int64_t wrow = gk;
          if constexpr (S2)
            wrow = (int64_t)dc.tap(cs, idiv<POW2>(gk, cs.d_cout)).widx *
                       cs.Cout + imod<POW2>(gk, cs.d_cout);
          return &WT[wrow * cs.Cin];
        },
        cs.Cin, n0, k0, K);
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    __syncthreads();
  }
  dgrad_store<POW2>(wc, acc, DX, cs, dc, m0, n0);
}

// ---------------------------------------------------------------------------
// double-buffered pure-glds dgrad (see k_conv_fwd_db; all-pow2 shapes only):
// the weight comes pre-transposed to [Cin, KH*KW*Cout] so B rows are
// k-contiguous; with S2 the compacted parity-class k index remaps into the
// full column space. One body for the 128x64 kernel and the wide forms, on
// two buffer pairs (DB) or one; its pointers take their __restrict__ from the
// kernels (see the epilogues' note).
template <typename T, bool S2, bool S1, bool DB, typename S = TileStd>
DEV void conv_dgrad_glds_tile(const T* DY, const T* WT2D, T* DX,
                              const T* zero16, const ConvShape& cs) {
  const DgradClass<S2> dc(cs);
  const int M = dc.M, K = dc.K;
  const int KFULL = cs.KH * cs.KW * cs.Cout;
  int tm_, tn_;
  conv_tile_order(cs, tm_, tn_);
  const int m0 = tm_ * S::BM;
  const int n0 = tn_ * S::BN;
  const WaveCoordT<S> wc;
  f32x4 acc[S::FM][S::FN] = {};

  // one LDS object per buffer, named statically in the 2x-unrolled k-loop;
  // the single-buffer form never touches the second pair, which then takes
  // no LDS
  __shared__ alignas(16) T As0[S::BM * BK], As1[DB ? S::BM * BK : 8];
  __shared__ alignas(16) T Bs0[S::BN * BK], Bs1[DB ? S::BN * BK : 8];
  conv_db_kloop<DB>(
      As0, As1, Bs0, Bs1, wc, acc, DY, cs.d_ow.lg, cs.d_cout.lg, WT2D,
      (int64_t)KFULL, cs.Cin, m0, n0, K, zero16,
      // d_hw / d_w hold the per-class (Hc*Wc, Wc) divisors under S2
      [&](int gm, int64_t& noff, int& p, int& q) {
        const int n = gm >> cs.d_hw.lg;
        const int rem = gm & (dc.Hc * dc.Wc - 1);
        int ih = rem >> cs.d_w.lg, iw = rem & (dc.Wc - 1);
        if constexpr (S2) {
          // th = ih + PH - kh is even by construction: oh = p - khi
          p = (2 * ih + dc.cls_a + cs.PH - dc.start_h) >> 1;
          q = (2 * iw + dc.cls_b + cs.PW - dc.start_w) >> 1;
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
          const DgradTap t = dc.tap(cs, kidx);
          dh = t.khi;
          dw = t.kwi;
          bcol = (t.widx << cs.d_cout.lg) + c;
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
  dgrad_store<true>(wc, acc, DX, cs, dc, m0, n0);
}

template <typename T, bool S2 = false, bool S1 = false>
__launch_bounds__(THREADS)
__global__ void k_conv_dgrad_db(const T* __restrict__ DY,
                                const T* __restrict__ WT2D,
                                T* __restrict__ DX,
                                const T* __restrict__ zero16, ConvShape cs) {
  conv_dgrad_glds_tile<T, S2, S1, true>(DY, WT2D, DX, zero16, cs);
}

// the 128x128 tile (TileWide, see k_conv_fwd_db_wide) for Cin % 128 == 0, as
// double buffer (64 KB LDS) and on one buffer pair (32 KB, 3 blocks per CU)
template <bool S2 = false, bool S1 = false>
__launch_bounds__(THREADS, 2)
__global__ void k_conv_dgrad_db_wide(const bf16* __restrict__ DY,
                                     const bf16* __restrict__ WT2D,
                                     bf16* __restrict__ DX,
                                     const bf16* __restrict__ zero16,
                                     ConvShape cs) {
  conv_dgrad_glds_tile<bf16, S2, S1, true, TileWide>(DY, WT2D, DX, zero16, cs);
}
template <bool S2 = false, bool S1 = false>
__launch_bounds__(THREADS, 3)
__global__ void k_conv_dgrad_sb_wide(const bf16* __restrict__ DY,
                                     const bf16* __restrict__ WT2D,
                                     bf16* __restrict__ DX,
                                     const bf16* __restrict__ zero16,
                                     ConvShape cs) {
  conv_dgrad_glds_tile<bf16, S2, S1, false, TileWide>(DY, WT2D, DX, zero16,
                                                      cs);
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
  // the gathered-x A operand [Kout, M] is re-read gridDim.y times
  conv_tile_order(cs, tr_, tn_);
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

  for (int k0 = m_begin; k0 < m_end; k0 += BK) {
    // ---- stage A^T: x rows ci-contiguous, scatter into As[ko][m] ----
#pragma unroll 1  // full unroll quadruples live address state (spills)
    for (int c = threadIdx.x; c < BK * (BM / V); c += THREADS) {
      int mm = c / (BM / V);
      int rr = (c % (BM / V)) * V;
      int gm = k0 + mm;
      int gr = r0 + rr;
      Pack16<T> v = {};
      if (gm < m_end && gr < Kout)
        v = fwd_gather16<POW2>(X, cs, fwd_row<POW2>(cs, gm), gr, Kout);
#pragma unroll
      for (int j = 0; j < V; ++j)
        As[lds_off<T>(rr + j, mm)] = v.e[j];
    }
    // dy[m][co] -> Bs[co][m]
    stage_b_transposed(
        Bs, [&](int gm) { return &DY[(int64_t)gm * cs.Cout]; }, cs.Cout, n0,
        k0, m_end);
    __syncthreads();
    mfma_compute_tile(As, Bs, wc, acc);
    if (colsum) bsum += colsum_tile_partial(Bs);
    __syncthreads();
  }
  float* out = wgrad_slab_store(wc, acc, DW, cs, Kout, bias_row, r0, n0);
  if (colsum) wgrad_colsum_store(out, cs, Kout, n0, bsum);
}

// ---------------------------------------------------------------------------
// vector-guaranteed wgrad (all-pow2 shape, Cin%V==0, Cout%V==0, 16B-aligned
// tensors; fp32 only -- bf16 takes k_conv_wgrad_tr): stages in three phases
// -- addresses (zero-page for OOB/padding), then all 16B loads, then the LDS
// scatter -- so RA+RB global loads stay in flight.
// The generic kernel's `#pragma unroll 1` staging (needed there to avoid
// 221-256 VGPR spills from per-iteration gather state) serializes to one
// load in flight per wave; holding only pointers between phases keeps the
// live state at ~24 VGPR.
// Software-pipelined (T14 rotate): tile t's registers are written to LDS,
// then tile t+1's loads are ISSUED into the same (now dead) registers before
// tile t's MFMA phase -- the gather latency lands under the MFMAs instead of
// being exposed at the head of every chunk (the attention kernels' TStage
// split, applied here).
// ---------------------------------------------------------------------------
template <typename T>
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
  conv_tile_order(cs, tr_, tn_);
  const int r0 = tr_ * BM;
  const int n0 = tn_ * BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoord wc;
  f32x4 acc[FM][FN] = {};
  const bool colsum = bias_row && tr_ == 0;  // see k_conv_wgrad
  float bsum = 0.0f;
  using VecT = Pack16<T>;

  VecT va[RA], vb[RB];
  auto load_tile = [&](int k0) {
    const T* asrc[RA];
#pragma unroll
    for (int it = 0; it < RA; ++it) {
      int c = threadIdx.x + it * THREADS;
      int mm = c / (BM / V);
      int rr = (c % (BM / V)) * V;
      int gm = k0 + mm, gr = r0 + rr;
      asrc[it] = gm < m_end && gr < Kout
                     ? fwd_src<true>(X, cs, fwd_row<true>(cs, gm), gr, zero16)
                     : zero16;
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
#pragma unroll
    for (int it = 0; it < RA; ++it) {
      int c = threadIdx.x + it * THREADS;
      int mm = c / (BM / V);
      int rr = (c % (BM / V)) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) As[lds_off<T>(rr + j, mm)] = va[it].e[j];
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
  float* out = wgrad_slab_store(wc, acc, DW, cs, Kout, bias_row, r0, n0);
  if (colsum) wgrad_colsum_store(out, cs, Kout, n0, bsum);
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
// Same gate as k_conv_wgrad_vec: all-pow2 shape, Cin%8 == Cout%8 == 0,
// 16B-aligned tensors. Double-buffered k-loop (48 KB LDS, 3 blocks/CU): it
// measured 3-5% ahead of the single-buffer form (24 KB) on the WRN shapes.
//
// One body for both block tiles (S) and both bufferings (DB; As1 / Bs1 are
// unused on one buffer pair). The A image is [BK][S::BM] with S::BM == 128;
// B is [BK][S::BN], 8 or 16 chunks per k-row. Chunk order, k-steps and the
// MFMA sequence per output element do not depend on S or DB, so dw and db
// are bitwise the same on every form for the same split count.
// ---------------------------------------------------------------------------
template <bool DB, typename S>
DEV void conv_wgrad_tr_tile(bf16* As0, bf16* As1, bf16* Bs0, bf16* Bs1,
                            const bf16* __restrict__ X,
                            const bf16* __restrict__ DY,
                            float* __restrict__ DW,
                            const bf16* __restrict__ zero16,
                            const ConvShape& cs, int bias_row) {
  constexpr int FM = S::FM, FN = S::FN;
  constexpr int ACH = S::BM / 8, BCH = S::BN / 8;   // 16-byte chunks per k-row
  static_assert(ACH == 16, "the hoisted A decode below is for 128-row tiles");
  static_assert(S::WAVES_M == 2, "bias row: wm selects half the fragments");
  constexpr int NA = glds_kmajor_count<ACH>();   // A glds per wave (4)
  constexpr int NPER = NA + glds_kmajor_count<BCH>();
  constexpr int NBF = FN / S::WAVES_M;   // bias-row fragments per wave
  const int M = cs.N * cs.OH * cs.OW;
  const int Kout = cs.KH * cs.KW * cs.Cin;
  int tr_, tn_;
  conv_tile_order(cs, tr_, tn_);
  const int r0 = tr_ * S::BM;
  const int n0 = tn_ * S::BN;
  const int m_begin = (int)((int64_t)M * blockIdx.z / gridDim.z);
  const int m_end = (int)((int64_t)M * (blockIdx.z + 1) / gridDim.z);
  const WaveCoordT<S> wc;
  const int wm = wc.wid / S::WAVES_N;
  f32x4 acc[FM][FN] = {};
  // bias gradient (see k_conv_wgrad): the dy fragments are already in
  // registers, so tile-row 0 sums them with all-ones MFMAs, one per k-step
  // and fragment; wave (wm, wn) takes the NBF fragments from column
  // wcol0 + 16*NBF*wm on, half of its wave tile
  const bool colsum = bias_row && tr_ == 0;
  f32x4 bacc[NBF] = {};
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
    glds_stage_kmajor<ACH>(a_img, wc,
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
    glds_stage_kmajor<BCH>(b_img, wc,
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
        a[fm] = tr_frag_issue<ACH>(a_img, ks * 32, wc.wrow0 + fm * 16,
                                   wc.lane);
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        b[fn] = tr_frag_issue<BCH>(b_img, ks * 32, wc.wcol0 + fn * 16,
                                   wc.lane);
      tr_frags_wait<S>(a, b);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[fm].get(), b[fn].get(), acc[fm][fn], 0, 0, 0);
      if (colsum) {
#pragma unroll
        for (int t = 0; t < NBF; ++t)
          bacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ones, wm ? b[NBF + t].get() : b[t].get(), bacc[t], 0, 0, 0);
      }
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
  if constexpr (DB) {
    if (m_begin < m_end) stage(m_begin, As0, Bs0);
    for (int k0 = m_begin; k0 < m_end; k0 += 2 * BK) {
      step(k0, As0, Bs0, As1, Bs1);
      if (k0 + BK < m_end) step(k0 + BK, As1, Bs1, As0, Bs0);
    }
  } else {
    // one buffer pair: half the LDS, one more resident block, no overlap
    // inside a block
    for (int k0 = m_begin; k0 < m_end; k0 += BK) {
      stage(k0, As0, Bs0);
      wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      compute(As0, Bs0);
      __builtin_amdgcn_s_barrier();
    }
  }

  float* out = wgrad_slab_store(wc, acc, DW, cs, Kout, bias_row, r0, n0);
  if (colsum) wgrad_biasrow_store<S>(out, wc, bacc, cs, Kout, n0);
}

__launch_bounds__(THREADS, 2)  // <=256 regs: MFMA accumulators stay in VGPRs
__global__ void k_conv_wgrad_tr(const bf16* __restrict__ X,
                                const bf16* __restrict__ DY,
                                float* __restrict__ DW,
                                const bf16* __restrict__ zero16, ConvShape cs,
                                int bias_row) {
  // one LDS object per buffer, named statically in the 2x-unrolled k-loop
  __shared__ alignas(16) bf16 As0[BK * BM], As1[BK * BM];  // [m][(kh,kw,ci)]
  __shared__ alignas(16) bf16 Bs0[BK * BN], Bs1[BK * BN];  // [m][co]
  conv_wgrad_tr_tile<true, TileStd>(As0, As1, Bs0, Bs1, X, DY, DW, zero16, cs,
                                    bias_row);
}

// the 128x128 tile (TileWide) of k_conv_wgrad_tr for Cout % 128 == 0: one
// transposed read per MFMA where the 128x64 tile issues 1.5, 32 KB of images
// per 2.1 MFLOP chunk instead of 24 KB per 1.05, and the gathered-x image
// with its (n, oh, ow) decode is fetched once per 128 output channels. The B
// image takes the 16-chunk layout A has. DB: 64 KB LDS, 2 blocks per CU;
// one buffer pair: 32 KB, capped at the 168 registers of 3 waves per SIMD.
template <bool DB>
__launch_bounds__(THREADS, DB ? 2 : 3)
__global__ void k_conv_wgrad_tr_wide(const bf16* __restrict__ X,
                                     const bf16* __restrict__ DY,
                                     float* __restrict__ DW,
                                     const bf16* __restrict__ zero16,
                                     ConvShape cs, int bias_row) {
  constexpr int WBM = TileWide::BM, WBN = TileWide::BN;
  if constexpr (DB) {
    __shared__ alignas(16) bf16 As0[BK * WBM], As1[BK * WBM];
    __shared__ alignas(16) bf16 Bs0[BK * WBN], Bs1[BK * WBN];
    conv_wgrad_tr_tile<true, TileWide>(As0, As1, Bs0, Bs1, X, DY, DW, zero16,
                                       cs, bias_row);
  } else {
    __shared__ alignas(16) bf16 As0[BK * WBM], Bs0[BK * WBN];
    conv_wgrad_tr_tile<false, TileWide>(As0, As0, Bs0, Bs0, X, DY, DW, zero16,
                                        cs, bias_row);
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
// launchers
// ---------------------------------------------------------------------------
static bool all_pow2(const ConvShape& cs) {
  return cs.d_ohow.lg >= 0 && cs.d_ow.lg >= 0 && cs.d_cin.lg >= 0 &&
         cs.d_hw.lg >= 0 && cs.d_w.lg >= 0 && cs.d_cout.lg >= 0;
}

// 16-byte vector / LDS-DMA access to an NHWC tensor with this many channels
static bool vec_ok(DT dt, const void* ptr, int channels) {
  return channels % vec_elems(dt) == 0 && ptr_aligned16(ptr);
}

// integer environment switch (callers read it once)
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// TNN_FWD_DB=0 routes fwd and dgrad back to the register-staged /
// single-buffer kernels, so both can be compared from one build
static bool db_on() {
  static const bool on = env_int("TNN_FWD_DB", 1) != 0;
  return on;
}

// k-loop length up to which the forward double buffer is used. Past it bf16
// takes the single-buffer form of the same DMA-staged tile; fp32 falls back
// to k_conv_fwd.
static int fwd_db_maxk() {
  static const int maxk = env_int("TNN_DB_MAXK", 2304);
  return maxk;
}

// TNN_CONV_WIDE: 0 never takes the 128x128 tile (TileWide), 1 (default)
// chooses per shape, 2 takes it wherever it is eligible
static int wide_mode() {
  static const int mode = env_int("TNN_CONV_WIDE", 1);
  return mode;
}
// A/B switch for the wide kernels' buffering: 0 (default) per shape, 1 always
// the double buffer, 2 always one buffer pair
static int wide_buf() {
  static const int buf = env_int("TNN_CONV_WIDE_BUF", 0);
  return buf;
}

// rows of the fused-statistics partials [rows][2][Cout]: one per m-tile (both
// block tiles are 128 rows tall)
int conv2d_fwd_stats_rows(const ConvShape& cs) {
  static_assert(TileWide::BM == BM, "one m-tile height for the partials");
  return ceil_div(cs.N * cs.OH * cs.OW, BM);
}

// The wide tile is eligible for a bf16 GEMM view [M, N, K] on the DMA-staged
// route when N % 128 == 0 (no N tail). What auto does with an eligible shape
// was fixed from the per-shape table in profiles/prof_wrn_conv_wide.md
// (slowest wide run against fastest 128x64 run); `tiles` counts the 128x128
// tiles of the whole launch.
enum class Wide { NO, DB, SB };
constexpr int WIDE_MIN_TILES = 512;   // smallest grid measured (and ahead)
constexpr int WIDE_FWD_DB_MINK = 2048;
constexpr int WIDE_DGRAD_SB_MAXK = 1152;
static Wide wide_pick(bool eligible, int tiles, bool take, bool single) {
  if (!eligible || wide_mode() == 0) return Wide::NO;
  if (wide_mode() == 1 && !(take && tiles >= WIDE_MIN_TILES)) return Wide::NO;
  if (wide_buf() != 0) single = wide_buf() == 2;
  return single ? Wide::SB : Wide::DB;
}
// forward, K = KH*KW*Cin:
//   one n-tile (Cout == 128)   one buffer pair wins 8-9 %, and with fused
//                              statistics 5-6 % (g1: 125.5-126.8 -> 118.8-
//                              119.4 us, g1 entry 53.7-54.1 -> 50.8-52.0,
//                              profiles/prof_wrn_grad_sink.md) now that the
//                              statistics are slab partials; with atomics the
//                              wide tile lost there (148 -> 190 us)
//   more n-tiles               the double buffer wins 11-26 % from K = 2304
//                              up; below that (K <= 1152) nothing wins
// The choice does not depend on whether statistics are fused.
static Wide fwd_wide(DT dt, bool have_wt2, const ConvShape& cs) {
  const int nt = cs.Cout / TileWide::BN;
  const int K = cs.KH * cs.KW * cs.Cin;
  const bool take = nt == 1 || K >= WIDE_FWD_DB_MINK;
  return wide_pick(
      have_wt2 && dt == DT::BF16 && cs.Cout % TileWide::BN == 0,
      ceil_div(cs.N * cs.OH * cs.OW, TileWide::BM) * nt, take, nt == 1);
}
// dgrad, K = taps * Cout with the taps of one parity class where the route is
// parity: wide wins or ties on every measured shape (5-43 %), on one buffer
// pair up to K = 1152 and double-buffered from K = 2048 up
static Wide dgrad_wide(DT dt, bool have_wt2d, bool s2, const ConvShape& cs) {
  const int M = s2 ? cs.N * (cs.H / 2) * (cs.W / 2) : cs.N * cs.H * cs.W;
  const int taps =
      s2 ? ((cs.KH + 1) / 2) * ((cs.KW + 1) / 2) : cs.KH * cs.KW;
  return wide_pick(
      have_wt2d && dt == DT::BF16 && cs.Cin % TileWide::BN == 0,
      ceil_div(M, TileWide::BM) * (cs.Cin / TileWide::BN) * (s2 ? 4 : 1),
      true, taps * cs.Cout <= WIDE_DGRAD_SB_MAXK);
}

template <typename... KArgs, typename... Args>
static void launch(void (*kern)(KArgs...), dim3 grid, hipStream_t s,
                   Args... args) {
  hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, args...);
}

// true: the launcher wants the [Cout][K] weight and takes a DMA-staged
// kernel, which also carries the fused statistics epilogue
bool conv2d_fwd_wants_db(DT dt, const void* x, const ConvShape& cs) {
  if (!db_on()) return false;
  if (dt == DT::F32 && cs.KH * cs.KW * cs.Cin > fwd_db_maxk()) return false;
  return all_pow2(cs) && vec_ok(dt, x, cs.Cin);
}

// out[b][c][r] = in[b][r][c]
static void transpose2d_launch(DT dt, const void* in, void* out, int batch,
                               int rows, int cols, hipStream_t s) {
  dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_transpose2d_tiled<T>, grid, dim3(256), 0, s,
                       (const T*)in, (T*)out, rows, cols);
  });
}

void transpose_w_fwd_launch(DT dt, const void* w, void* w_t2, int KHW, int Cin,
                            int Cout, hipStream_t s) {
  // [KHW*Cin, Cout] -> [Cout, KHW*Cin] is a plain 2D transpose
  transpose2d_launch(dt, w, w_t2, 1, KHW * Cin, Cout, s);
}

void transpose_w_launch(DT dt, const void* w, void* w_t, int KH, int KW,
                        int Cin, int Cout, hipStream_t s) {
  // batched [Cin, Cout] -> [Cout, Cin] transpose per (kh,kw) slice
  transpose2d_launch(dt, w, w_t, KH * KW, Cin, Cout, s);
}

void transpose_w_dgrad_launch(DT dt, const void* w, void* w_t2d, int KHW,
                              int Cin, int Cout, hipStream_t s) {
  const bool vec = vec_ok(dt, w, Cout);
  int64_t n = (int64_t)KHW * Cin * (vec ? Cout / vec_elems(dt) : Cout);
  int blocks = (int)((n + 255) / 256);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto kern = vec ? k_transpose_w_dgrad_vec<T> : k_transpose_w_dgrad<T>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, (const T*)w,
                       (T*)w_t2d, KHW, Cin, Cout);
  });
}

// Route, first match (K = KH*KW*Cin; w_t2 is passed iff conv2d_fwd_wants_db:
// switch on, all-pow2, vector gate, and for fp32 K <= TNN_DB_MAXK; wide: bf16,
// Cout % 128 == 0 and TNN_CONV_WIDE says so, see fwd_wide):
//   w_t2, wide, Cout == 128       k_conv_fwd_sb_wide<stats>
//   w_t2, wide                    k_conv_fwd_db_wide<stats>
//   w_t2, bf16, K > TNN_DB_MAXK   k_conv_fwd_sb<stats>
//   w_t2                          k_conv_fwd_db<T, stats>
//   all-pow2 and vector gate      k_conv_fwd<T, true, true>    (A by LDS-DMA)
//   all-pow2                      k_conv_fwd<T, true, false>
//   otherwise                     k_conv_fwd<T, false, false>
// stats is honoured on the w_t2 routes only.
enum class FwdRoute { SB_WIDE, DB_WIDE, SB, DB, GLDS, POW2, GENERIC };
static FwdRoute fwd_route(DT dt, const void* x, bool have_wt2,
                          const ConvShape& cs, bool stats) {
  if (have_wt2) {
    const Wide wide = fwd_wide(dt, true, cs);
    if (wide != Wide::NO)
      return wide == Wide::SB ? FwdRoute::SB_WIDE : FwdRoute::DB_WIDE;
    const bool long_k =
        dt == DT::BF16 && cs.KH * cs.KW * cs.Cin > fwd_db_maxk();
    return long_k ? FwdRoute::SB : FwdRoute::DB;
  }
  if (!all_pow2(cs)) return FwdRoute::GENERIC;
  return vec_ok(dt, x, cs.Cin) ? FwdRoute::GLDS : FwdRoute::POW2;
}

const char* conv2d_fwd_route(DT dt, const void* x, const ConvShape& cs,
                             bool stats) {
  const bool db = conv2d_fwd_wants_db(dt, x, cs);
  switch (fwd_route(dt, x, db, cs, db && stats)) {
    case FwdRoute::SB_WIDE: return "k_conv_fwd_sb_wide";
    case FwdRoute::DB_WIDE: return "k_conv_fwd_db_wide";
    case FwdRoute::SB: return "k_conv_fwd_sb";
    case FwdRoute::DB: return "k_conv_fwd_db";
    case FwdRoute::GLDS: return "k_conv_fwd<pow2, glds>";
    case FwdRoute::POW2: return "k_conv_fwd<pow2>";
    default: return "k_conv_fwd";
  }
}

void conv2d_fwd_launch(DT dt, const void* x, const void* w, const void* w_t2,
                       const void* bias, void* y, const void* zero16,
                       float* stats, const ConvShape& cs, bool relu,
                       hipStream_t s) {
  int M = cs.N * cs.OH * cs.OW;
  dim3 grid(ceil_div(M, BM), ceil_div(cs.Cout, BN));
  dim3 grid_wide(ceil_div(M, TileWide::BM), ceil_div(cs.Cout, TileWide::BN));
  int act = relu ? ACT_RELU : ACT_LINEAR;
  const FwdRoute route =
      fwd_route(dt, x, w_t2 != nullptr, cs, stats != nullptr);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto X = (const T*)x;
    auto B = (const T*)bias;
    auto Y = (T*)y;
    auto Z = (const T*)zero16;
    if constexpr (sizeof(T) == 2) {
      // bf16 only (fwd_route never names these for fp32)
      if (route == FwdRoute::SB_WIDE)
        return launch(
            stats ? k_conv_fwd_sb_wide<true> : k_conv_fwd_sb_wide<false>,
            grid_wide, s, X, (const T*)w_t2, B, Y, Z, cs, act, stats);
      if (route == FwdRoute::DB_WIDE)
        return launch(
            stats ? k_conv_fwd_db_wide<true> : k_conv_fwd_db_wide<false>,
            grid_wide, s, X, (const T*)w_t2, B, Y, Z, cs, act, stats);
      if (route == FwdRoute::SB)
        return launch(stats ? k_conv_fwd_sb<true> : k_conv_fwd_sb<false>,
                      grid, s, X, (const T*)w_t2, B, Y, Z, cs, act, stats);
    }
    if (route == FwdRoute::DB)
      return launch(stats ? k_conv_fwd_db<T, true> : k_conv_fwd_db<T, false>,
                    grid, s, X, (const T*)w_t2, B, Y, Z, cs, act, stats);
    launch(route == FwdRoute::GLDS
               ? k_conv_fwd<T, true, true>
               : (route == FwdRoute::POW2 ? k_conv_fwd<T, true, false>
                                          : k_conv_fwd<T, false, false>),
           grid, s, X, (const T*)w, B, Y, Z, cs, act);
  });
}

bool conv2d_dgrad_wants_db(DT dt, const void* dy, const ConvShape& cs) {
  if (!db_on()) return false;
  // dgrad ties-or-wins with the double buffer up to here
  static const int maxk = env_int("TNN_DB_MAXK_DGRAD", 4608);
  return cs.KH * cs.KW * cs.Cout <= maxk && all_pow2(cs) &&
         vec_ok(dt, dy, cs.Cout);
}

// the parity route's per-class shape; false where the route does not apply.
// KW <= 4: a class then has at most 2 taps across, which is all that
// DgradClass::tap decodes; wider kernels take the any-stride forms.
static bool dgrad_parity(const ConvShape& cs, ConvShape& cs2) {
  bool s2 = all_pow2(cs) && cs.SH == 2 && cs.SW == 2 && cs.H % 2 == 0 &&
            cs.W % 2 == 0 && cs.KW <= 4;
  cs2 = cs;
  if (s2) {
    cs2.d_hw.set((cs.H / 2) * (cs.W / 2));
    cs2.d_w.set(cs.W / 2);
    s2 = cs2.d_hw.lg >= 0 && cs2.d_w.lg >= 0;
  }
  return s2;
}

// Route, first match (w_t2d is passed iff conv2d_dgrad_wants_db: switch on,
// all-pow2, vector gate, KH*KW*Cout <= TNN_DB_MAXK_DGRAD; else w_t).
// parity = all-pow2, stride 2x2, even H and W, KW <= 4, pow2 per-class
// divisors: 4 classes in grid.z over an M/4-row problem (see DgradClass), cs
// with the per-class divisors.
// wide: bf16, Cin % 128 == 0 and TNN_CONV_WIDE says so (dgrad_wide); the wide
// routes take the same parity / stride-1 / any-stride forms:
//   w_t2d, wide, K <= 1152        k_conv_dgrad_sb_wide<S2, S1>
//   w_t2d, wide                   k_conv_dgrad_db_wide<S2, S1>
//   w_t2d, parity                 k_conv_dgrad_db<T, S2>
//   w_t2d, stride 1x1             k_conv_dgrad_db<T, -, S1>
//   w_t2d                         k_conv_dgrad_db<T>           (any stride)
//   vector gate, parity           k_conv_dgrad<T, true, true, S2>
//   vector gate, stride 1x1       k_conv_dgrad<T, true, true, -, S1>
//   vector gate                   k_conv_dgrad<T, true, true>
//   all-pow2                      k_conv_dgrad<T, true, false>
//   otherwise                     k_conv_dgrad<T, false, false>
const char* conv2d_dgrad_route(DT dt, const void* dy, const ConvShape& cs) {
  ConvShape cs2;
  const bool s2 = dgrad_parity(cs, cs2);
  const bool s1 = cs.SH == 1 && cs.SW == 1;
  const bool p2 = all_pow2(cs);
  if (conv2d_dgrad_wants_db(dt, dy, cs)) {
    const Wide wide = dgrad_wide(dt, true, s2, cs);
    if (wide == Wide::SB)
      return s2 ? "k_conv_dgrad_sb_wide<S2>"
                : (s1 ? "k_conv_dgrad_sb_wide<S1>" : "k_conv_dgrad_sb_wide");
    if (wide == Wide::DB)
      return s2 ? "k_conv_dgrad_db_wide<S2>"
                : (s1 ? "k_conv_dgrad_db_wide<S1>" : "k_conv_dgrad_db_wide");
    return s2 ? "k_conv_dgrad_db<S2>"
              : (s1 ? "k_conv_dgrad_db<S1>" : "k_conv_dgrad_db");
  }
  if (p2 && vec_ok(dt, dy, cs.Cout))
    return s2 ? "k_conv_dgrad<pow2, glds, S2>"
              : (s1 ? "k_conv_dgrad<pow2, glds, S1>"
                    : "k_conv_dgrad<pow2, glds>");
  return p2 ? "k_conv_dgrad<pow2>" : "k_conv_dgrad";
}

void conv2d_dgrad_launch(DT dt, const void* dy, const void* w_t,
                         const void* w_t2d, void* dx, const void* zero16,
                         const ConvShape& cs, hipStream_t s) {
  int M = cs.N * cs.H * cs.W;
  dim3 grid(ceil_div(M, BM), ceil_div(cs.Cin, BN));
  bool p2 = all_pow2(cs);
  bool g = p2 && vec_ok(dt, dy, cs.Cout);
  bool s1 = cs.SH == 1 && cs.SW == 1;
  ConvShape cs2;
  bool s2 = dgrad_parity(cs, cs2);
  int Mc = cs.N * (cs.H / 2) * (cs.W / 2);   // rows of one parity class
  dim3 grid_s2(ceil_div(Mc, BM), ceil_div(cs.Cin, BN), 4);
  const Wide wide = dgrad_wide(dt, w_t2d != nullptr, s2, cs);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto DY = (const T*)dy;
    auto DX = (T*)dx;
    auto Z = (const T*)zero16;
    if constexpr (sizeof(T) == 2) {
      if (wide != Wide::NO) {   // bf16 only
        auto WT = (const T*)w_t2d;
        constexpr int WBM = TileWide::BM, WBN = TileWide::BN;
        const bool sb = wide == Wide::SB;
        if (s2)
          return launch(sb ? k_conv_dgrad_sb_wide<true>
                           : k_conv_dgrad_db_wide<true>,
                        dim3(ceil_div(Mc, WBM), cs.Cin / WBN, 4), s, DY, WT,
                        DX, Z, cs2);
        dim3 gw(ceil_div(M, WBM), cs.Cin / WBN);
        if (s1)
          return launch(sb ? k_conv_dgrad_sb_wide<false, true>
                           : k_conv_dgrad_db_wide<false, true>,
                        gw, s, DY, WT, DX, Z, cs);
        return launch(sb ? k_conv_dgrad_sb_wide<> : k_conv_dgrad_db_wide<>,
                      gw, s, DY, WT, DX, Z, cs);
      }
    }
    if (w_t2d) {
      auto WT = (const T*)w_t2d;
      if (s2)
        return launch(k_conv_dgrad_db<T, true>, grid_s2, s, DY, WT, DX, Z,
                      cs2);
      return launch(s1 ? k_conv_dgrad_db<T, false, true> : k_conv_dgrad_db<T>,
                    grid, s, DY, WT, DX, Z, cs);
    }
    auto WT = (const T*)w_t;
    if (g && s2)
      return launch(k_conv_dgrad<T, true, true, true>, grid_s2, s, DY, WT, DX,
                    Z, cs2);
    launch(g ? (s1 ? k_conv_dgrad<T, true, true, false, true>
                   : k_conv_dgrad<T, true, true>)
             : (p2 ? k_conv_dgrad<T, true, false>
                   : k_conv_dgrad<T, false, false>),
           grid, s, DY, WT, DX, Z, cs);
  });
}

// TNN_WGRAD_WIDE: 0 never takes the 128x128 tile for wgrad, 1 (default)
// chooses per shape, 2 takes it wherever it is eligible. TNN_WGRAD_WIDE_BUF:
// 0 (default) per shape, 1 always the double buffer, 2 always one buffer
// pair. Separate from TNN_CONV_WIDE, which keeps steering fwd and dgrad only.
static int wgrad_wide_mode() {
  static const int mode = env_int("TNN_WGRAD_WIDE", 1);
  return mode;
}
static int wgrad_wide_buf() {
  static const int buf = env_int("TNN_WGRAD_WIDE_BUF", 0);
  return buf;
}
// TNN_WGRAD_SPLITS=<z> pins the split count of every wgrad launch (clamped to
// [1, ceil(M / (4*BK))]); 0 or unset leaves it to the policy below
static int wgrad_splits_pin() {
  static const int z = env_int("TNN_WGRAD_SPLITS", 0);
  return z;
}

// Route, first match (vector gate: all-pow2, Cin and Cout multiples of the
// vector width, x and dy 16-byte aligned; wide: Cout % 128 == 0 and
// TNN_WGRAD_WIDE says so, see wgrad_wide):
//   vector gate, bf16, wide       k_conv_wgrad_tr_wide<db> or <sb>
//   vector gate, bf16             k_conv_wgrad_tr
//   vector gate, fp32             k_conv_wgrad_vec<float>
//   all-pow2                      k_conv_wgrad<T, true>
//   otherwise                     k_conv_wgrad<T, false>
// then the split-M reduce unless the kernel wrote dw_out directly. The route
// is a function of the shape, dtype and alignment only -- never of whether
// the bias row is asked for.
enum class WgradRoute { TR_WIDE_DB, TR_WIDE_SB, TR, VEC, POW2, GENERIC };

// What auto does with an eligible shape, from the per-shape table in
// profiles/prof_wrn_wgrad_wide.md (slowest wide timing against the fastest
// 128x64 timing, reduce included), `tiles` = 128x128 tiles of dw:
// in time saved:
//   grid size                   one resident wave ties or beats two on every
//                               shape and form (up to 30 %); two beat four
//   Cout == 128, Kout = 1152    (g1) both forms lose 2-12 % at every grid
//                               size: stays on k_conv_wgrad_tr
//   Cout == 128, Kout <= 144    (16->128 entry and 1x1) double buffer 28-31 %,
//                               one buffer pair 15-19 %
//   Cout >= 256, tiles <= 72    double buffer 4-21 %, one buffer pair 2-16 %
//   tiles = 144                 (g3) one buffer pair 8 %, the double buffer
//                               5 % (its 3 splits fill 432 of 512 slots)
// Shapes whose split cap leaves less than one resident wave of wide blocks
// were not measured and stay on the 128x64 tile, which makes more blocks.
constexpr int WGRAD_WIDE_WAVES = 1;
constexpr int WGRAD_WIDE_1TILE_MAXKOUT = 144;
constexpr int WGRAD_WIDE_SB_MINTILES = 144;
constexpr int WGRAD_WIDE_DB_SLOTS = 512, WGRAD_WIDE_SB_SLOTS = 768;
// TNN_WGRAD_WAVES=<n> sizes the wide grids to n resident waves (the sweep)
static int wgrad_wide_waves() {
  static const int n =
      std::max(env_int("TNN_WGRAD_WAVES", WGRAD_WIDE_WAVES), 1);
  return n;
}
static Wide wgrad_wide_auto(const ConvShape& cs) {
  const int Kout = cs.KH * cs.KW * cs.Cin;
  const int nt = cs.Cout / TileWide::BN;
  const int tiles = ceil_div(Kout, TileWide::BM) * nt;
  const int cap = ceil_div(cs.N * cs.OH * cs.OW, 4 * BK);
  if (nt == 1 && Kout > WGRAD_WIDE_1TILE_MAXKOUT) return Wide::NO;
  if (cap < WGRAD_WIDE_DB_SLOTS / tiles) return Wide::NO;
  return tiles >= WGRAD_WIDE_SB_MINTILES ? Wide::SB : Wide::DB;
}
static Wide wgrad_wide(const ConvShape& cs) {
  if (cs.Cout % TileWide::BN != 0 || wgrad_wide_mode() == 0) return Wide::NO;
  Wide pick = wgrad_wide_auto(cs);
  if (wgrad_wide_mode() == 1 && pick == Wide::NO) return Wide::NO;
  if (wgrad_wide_buf() != 0)
    pick = wgrad_wide_buf() == 2 ? Wide::SB : Wide::DB;
  else if (pick == Wide::NO)
    pick = Wide::DB;   // forced (mode 2) where auto would not go wide
  return pick;
}

static WgradRoute wgrad_route(DT dt, const void* x, const void* dy,
                              const ConvShape& cs) {
  const bool p2 = all_pow2(cs);
  if (p2 && vec_ok(dt, x, cs.Cin) && vec_ok(dt, dy, cs.Cout)) {
    if (dt != DT::BF16) return WgradRoute::VEC;
    const Wide wide = wgrad_wide(cs);
    if (wide == Wide::NO) return WgradRoute::TR;
    return wide == Wide::SB ? WgradRoute::TR_WIDE_SB : WgradRoute::TR_WIDE_DB;
  }
  return p2 ? WgradRoute::POW2 : WgradRoute::GENERIC;
}

// Split-M count of the launch wgrad_route names; the bindings size the slab
// workspace from it. 128x64 kernels: about 2048 blocks. Wide kernels: the
// grid is sized to the resident slots of their form (256 CUs x 2 blocks
// double-buffered, x 3 on one buffer pair) times WGRAD_WIDE_WAVES, rounded
// down -- every block writes its whole fp32 tile to a slab, so slab bytes are
// blocks x tile bytes, and 2048 blocks of 64 KB would double them.
int conv2d_wgrad_zsplits(DT dt, const void* x, const void* dy,
                         const ConvShape& cs) {
  const int M = cs.N * cs.OH * cs.OW;
  const int Kout = cs.KH * cs.KW * cs.Cin;
  const int cap = std::max(ceil_div(M, 4 * BK), 1);
  if (wgrad_splits_pin() > 0) return std::min(wgrad_splits_pin(), cap);
  const WgradRoute route = wgrad_route(dt, x, dy, cs);
  if (route == WgradRoute::TR_WIDE_DB || route == WgradRoute::TR_WIDE_SB) {
    const int base = ceil_div(Kout, TileWide::BM) * (cs.Cout / TileWide::BN);
    const int slots = (route == WgradRoute::TR_WIDE_DB ? WGRAD_WIDE_DB_SLOTS
                                                       : WGRAD_WIDE_SB_SLOTS) *
                      wgrad_wide_waves();
    return std::max(std::min(cap, slots / base), 1);
  }
  int base = ceil_div(Kout, BM) * ceil_div(cs.Cout, BN);
  int want = 2048;
  int z = base >= want ? 1 : std::min(cap, ceil_div(want, base));
  return std::max(z, 1);
}

const char* conv2d_wgrad_route(DT dt, const void* x, const void* dy,
                               const ConvShape& cs) {
  switch (wgrad_route(dt, x, dy, cs)) {
    case WgradRoute::TR_WIDE_DB: return "k_conv_wgrad_tr_wide<db>";
    case WgradRoute::TR_WIDE_SB: return "k_conv_wgrad_tr_wide<sb>";
    case WgradRoute::TR: return "k_conv_wgrad_tr";
    case WgradRoute::VEC: return "k_conv_wgrad_vec";
    case WgradRoute::POW2: return "k_conv_wgrad<pow2>";
    default: return "k_conv_wgrad";
  }
}

// z: conv2d_wgrad_zsplits of the same arguments (the workspace holds z slabs)
// sink: dw_out is a parameter's gradient buffer ([Kout][Cout] only) and the
// bias row, if asked for, goes to sink->db_out; sink->accumulate adds to what
// both hold. Same route, z and workspace: only the reduce's destinations
// differ. A sink always takes the workspace plus the reduce, also where
// z == 1 with fp32 output would write dw_out directly: the direct tile is
// [Kout+1][Cout] in one piece and cannot add to a gradient.
void conv2d_wgrad_launch(DT dt, const void* x, const void* dy, void* dw_out,
                         DT out_dt, float* ws, int z, const void* zero16,
                         const ConvShape& cs, bool bias, hipStream_t s,
                         const WgradSink* sink) {
  int Kout = cs.KH * cs.KW * cs.Cin;
  // bias: dw_out and every slab carry one more row, [Kout+1][Cout], whose
  // last row is the bias gradient sum_m dy (summed by the tile-row-0 blocks)
  const int bias_row = bias ? 1 : 0;
  // bf16 output always goes through the (casting) reduce; fp32 with z==1
  // writes the slab target directly
  bool direct = z == 1 && out_dt == DT::F32 && !sink;
  float* target = direct ? (float*)dw_out : ws;
  dim3 grid(ceil_div(Kout, BM), ceil_div(cs.Cout, BN), z);
  const WgradRoute route = wgrad_route(dt, x, dy, cs);
  dispatch_dt(dt, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto X = (const T*)x;
    auto DY = (const T*)dy;
    auto Z = (const T*)zero16;
    if constexpr (sizeof(T) == 2) {
      // bf16 only (wgrad_route never names these for fp32)
      if (route == WgradRoute::TR_WIDE_DB || route == WgradRoute::TR_WIDE_SB)
        return launch(route == WgradRoute::TR_WIDE_DB
                          ? k_conv_wgrad_tr_wide<true>
                          : k_conv_wgrad_tr_wide<false>,
                      dim3(ceil_div(Kout, TileWide::BM),
                           cs.Cout / TileWide::BN, z),
                      s, X, DY, target, Z, cs, bias_row);
      if (route == WgradRoute::TR)
        return launch(k_conv_wgrad_tr, grid, s, X, DY, target, Z, cs,
                      bias_row);
    } else {
      if (route == WgradRoute::VEC)
        return launch(k_conv_wgrad_vec<T>, grid, s, X, DY, target, Z, cs,
                      bias_row);
    }
    launch(route == WgradRoute::POW2 ? k_conv_wgrad<T, true>
                                     : k_conv_wgrad<T, false>,
           grid, s, X, DY, target, cs, bias_row);
  });
  // the reduce kernel (and so dw's summation order) is chosen from dw's own
  // size: with Cout % 4 == 0 the extra row never changes dw's bits (else the
  // longer output can fall off the float4 reduce; still deterministic)
  if (!direct)
    splitk_reduce_launch(ws, dw_out, out_dt, z,
                         (int64_t)(Kout + bias_row) * cs.Cout, s,
                         (int64_t)Kout * cs.Cout,
                         sink && bias ? sink->db_out : nullptr,
                         (int64_t)Kout * cs.Cout, sink && sink->accumulate);
}

}  // namespace tnn
