// MFMA block-tile GEMM core shared by the dense GEMM and the implicit-GEMM
// convolution kernels (replaces reference cublasGemmEx call sites,
// src/math/cuda/gemm.cu:64, and the cuDNN-frontend conv graphs).
//
// Structure (cdna_hip_programming.md §5 canonical GEMM):
//   - 256 threads = 4 waves in a 2x2 grid; block tile BM=128 x BN=64, BK=64.
//   - A staged in LDS as [BM][BK] row-major; B staged TRANSPOSED as
//     [BN][BK] so both operands read contiguous k-vectors per lane.
//   - LDS banking: element (row, col) lives at byte
//     (col*sizeof(T)) ^ ((((row>>3)^row)&7)<<4) within its 128B+ row.
//     The XOR key mixes low AND mid row bits so BOTH access patterns are
//     spread across banks: fragment reads touch 16 consecutive rows
//     (key varies via row&7) and transpose-scatter writes touch rows at
//     stride 8 across lanes (key varies via row>>3). Plain +pad schemes
//     can't fix the scatter side: any 16B-aligned row stride puts an
//     8-row lane stride on one bank (measured 3e8 conflict cycles).
//   - bf16: v_mfma_f32_16x16x32_bf16; fp32: v_mfma_f32_16x16x4_f32
//     (exact f32 at the f32 vector rate — no xf32 on gfx950).
//   - Each wave owns a 64x32 sub-tile: 4x2 fragments, f32x4 accumulators.
//   - The block tile is a compile-time shape tag (TileShape). Everything
//     defaults to the geometry above; the bf16 DMA-staged conv kernels also
//     come in TileWide, 128x128 with 64x64 wave tiles (4x4 fragments), which
//     stages two thirds of the bytes per FLOP. Both shapes share BK, the
//     swizzled [rows][BK] image and the per-element MFMA sequence. The
//     k-major pieces of the bf16 wgrad (glds_stage_kmajor, tr_frags_wait)
//     take the same tag.
#pragma once

#include "common.h"

namespace tile {

constexpr int BK = 64, THREADS = 256;

template <int BM_, int BN_, int WAVES_M_ = 2, int WAVES_N_ = 2>
struct TileShape {
  static constexpr int BM = BM_, BN = BN_;
  static constexpr int WAVES_M = WAVES_M_, WAVES_N = WAVES_N_;  // wave grid
  static constexpr int WM = BM / WAVES_M;      // rows per wave
  static constexpr int WN = BN / WAVES_N;      // cols per wave
  static constexpr int FM = WM / 16;           // row fragments
  static constexpr int FN = WN / 16;           // col fragments
  static_assert(WAVES_M * WAVES_N * 64 == THREADS, "one wave per sub-tile");
  static_assert(WM % 16 == 0 && WN % 16 == 0, "whole 16x16 fragments");
};
using TileStd = TileShape<128, 64>;     // 64x32 wave tiles, 4x2 fragments
using TileWide = TileShape<128, 128>;   // 64x64 wave tiles, 4x4 fragments

// the default shape's numbers, for everything that does not take a tag
constexpr int BM = TileStd::BM, BN = TileStd::BN;
constexpr int WAVES_M = TileStd::WAVES_M, WAVES_N = TileStd::WAVES_N;
constexpr int WM = TileStd::WM;              // 64 rows per wave
constexpr int WN = TileStd::WN;              // 32 cols per wave
constexpr int FM = TileStd::FM;              // 4 row fragments
constexpr int FN = TileStd::FN;              // 2 col fragments

// 16-byte staging pack (dwordx4 load/store); ext_vector_type cannot hold
// the __hip_bfloat16 struct, an aligned POD array can.
template <typename T> struct alignas(16) Pack16 {
  T e[16 / sizeof(T)];
};

template <typename T>
DEV bool aligned16(const T* p) {
  return ((unsigned long long)(const void*)p & 15ull) == 0;
}

// 16 bytes of row_base[idx .. idx+V): one vector load when the span is
// inside [0, limit) and 16B-aligned, else element-wise with zero fill.
template <typename T>
DEV Pack16<T> load16_guarded(const T* row_base, int idx, int limit) {
  constexpr int V = 16 / sizeof(T);
  const T* src = row_base + idx;
  Pack16<T> v = {};
  if (idx + V <= limit && aligned16(src)) {
    v = *(const Pack16<T>*)src;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (idx + j < limit) v.e[j] = src[j];
  }
  return v;
}

// element offset of tile element (row, col) in the swizzled [rows][BK]
// image; the XOR only touches byte bits 4-6, so any 16B-aligned col keeps
// its vector contiguous and the swizzle stays inside the row.
template <typename T>
DEV int lds_off(int row, int col) {
  int byte = col * (int)sizeof(T);
  byte ^= ((((row >> 3) ^ row) & 7) << 4);
  return row * BK + byte / (int)sizeof(T);
}


template <typename T> struct LDSBytes {
  static constexpr int A = BM * BK * sizeof(T);
  static constexpr int B = BN * BK * sizeof(T);
  static constexpr int total = A + B;
};

// L2-locality tile remap (grouped ordering): dispatch-linear block ids
// sweep GM m-tiles x ALL n-tiles in panels, so a panel's A rows stay
// L2-resident while every B column streams once per panel — without
// this an [M,N,K] GEMM re-reads A (N/BN) times from HBM (measured: the
// fc1-shaped GEMM's whole runtime equals that traffic at 8 TB/s).
template <int GM>
DEV void tile_remap(int& tm, int& tn) {
  const int nbx = gridDim.x, nby = gridDim.y;
  const int id = blockIdx.y * nbx + blockIdx.x;  // dispatch order, x fastest
  const int per_group = GM * nby;
  const int group = id / per_group;
  const int first_m = group * GM;
  const int gm = min(nbx - first_m, GM);
  const int rem = id - group * per_group;
  tm = first_m + rem % gm;
  tn = rem / gm;
}

// XCD-aware variant: the dispatcher round-robins consecutive block ids
// over the 8 XCDs, so id%8 IS the XCD. Give each XCD a contiguous,
// grouped stripe of the tile space: panel reuse then hits the XCD's own
// (non-coherent) 4 MiB L2 instead of only the die-level L3.
template <int GM>
DEV void tile_remap_xcd(int& tm, int& tn) {
  const int nbx = gridDim.x, nby = gridDim.y;
  const int T = nbx * nby;
  const int id = blockIdx.y * nbx + blockIdx.x;
  // stripe permutation is a bijection only when 8 | T (every CNN-zoo
  // grid: pow2 tiles); otherwise keep dispatch order — a clamped
  // fallback here DUPLICATED one tile and dropped another per ragged
  // stripe, silently corrupting C
  const int lid = (T & 7) == 0 ? ((id & 7) * (T >> 3) + (id >> 3)) : id;
  const int per_group = GM * nby;
  const int group = lid / per_group;
  const int first_m = group * GM;
  const int gm = min(nbx - first_m, GM);
  const int rem = lid - group * per_group;
  tm = first_m + rem % gm;
  tn = rem / gm;
}

template <typename S = TileStd>
struct WaveCoordT {
  using Shape = S;
  int wid, lane, wrow0, wcol0;
  DEV WaveCoordT() {
    wid = threadIdx.x >> 6;
    lane = threadIdx.x & 63;
    wrow0 = (wid / S::WAVES_N) * S::WM;
    wcol0 = (wid % S::WAVES_N) * S::WN;
  }
};
using WaveCoord = WaveCoordT<>;

// ---- async global->LDS staging for the A tile (gfx950 global_load_lds) ---
// Writes the whole [BM][BK] swizzled image with 16B-per-lane DMA: each
// wave issues (BM*BK*sizeof(T))/4096 instructions, each filling a 1 KiB
// lane-linear LDS region. The swizzle therefore moves to the SOURCE
// address (guide rule 21): each lane asks AddrFn for the element that
// belongs at its linear LDS slot. Invalid lanes (image padding, M/K
// tails) point their source at a 16-byte zero page — no exec masking, no
// pre-zeroing pass (a masked glds lane would leave stale LDS bytes).
// AddrFn: (row_in_tile, col_elem) -> const T* (16B-aligned) or zero16.
template <typename T, int ROWS, typename AddrFn>
DEV void glds_stage(T* As, const WaveCoord& w, AddrFn&& addr) {
  constexpr int ROWB = BK * (int)sizeof(T);      // bytes per image row
  constexpr int RPK = 1024 / ROWB;               // rows per 1 KiB region
  constexpr int LPR = ROWB / 16;                 // lanes per row
  constexpr int NREG = ROWS * ROWB / 1024;       // 1 KiB regions in the tile
  constexpr int NPW = NREG / 4;                  // regions per wave
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const int j = w.wid * NPW + i;
    const int rl = RPK * j + w.lane / LPR;
    const int byte_in_row = (w.lane % LPR) * 16;
    const int kk = (byte_in_row ^ ((((rl >> 3) ^ rl) & 7) << 4)) /
                   (int)sizeof(T);
    const T* src = addr(rl, kk);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)
            &As[j * (1024 / (int)sizeof(T))],
        16, 0, 0);
  }
}

template <typename T, typename AddrFn>
DEV void glds_stage_a(T* As, const WaveCoord& w, AddrFn&& addr) {
  glds_stage<T, BM>(As, w, addr);
}

// glds instructions per wave for one ROWS-row tile (vmcnt bookkeeping)
template <typename T, int ROWS>
constexpr int glds_count() {
  return ROWS * (BK * (int)sizeof(T)) / 1024 / 4;
}

// counted s_waitcnt vmcnt(N): __syncthreads() with a glds in flight drains
// vmcnt(0) (guide: LDS-DMA is a pending LDS write on the VM counter), so
// double-buffered loops wait an explicit partial count + raw s_barrier.
template <int N>
DEV void wait_vmcnt() {
  static_assert(N == 0 || N == 4 || N == 6 || N == 8 || N == 12 ||
                N == 16 || N == 24,
                "add an asm literal for this count");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
}


// ---- MFMA tile compute: acc[FM][FN] += A_tile * B_tile^T-stored -----------
DEV void mfma_compute_tile(const bf16* As, const bf16* Bs, const WaveCoord& w,
                           f32x4 acc[FM][FN]) {
  const int r = w.lane & 15;            // fragment row/col within 16
#pragma unroll
  for (int ks = 0; ks < BK / 32; ++ks) {
    const int kb = ks * 32 + (w.lane >> 4) * 8;  // 8 bf16 per lane
    bf16x8 a[FM], b[FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
      a[fm] = *(const bf16x8*)&As[lds_off<bf16>(w.wrow0 + fm * 16 + r, kb)];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      b[fn] = *(const bf16x8*)&Bs[lds_off<bf16>(w.wcol0 + fn * 16 + r, kb)];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[fm], b[fn], acc[fm][fn], 0, 0, 0);
  }
}

DEV void mfma_compute_tile(const float* As, const float* Bs, const WaveCoord& w,
                           f32x4 acc[FM][FN]) {
  const int r = w.lane & 15;
  const int kq = w.lane >> 4;         // one f32 per lane per k-step of 4
#pragma unroll
  for (int ks = 0; ks < BK / 4; ++ks) {
    float a[FM], b[FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
      a[fm] = As[lds_off<float>(w.wrow0 + fm * 16 + r, ks * 4 + kq)];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      b[fn] = Bs[lds_off<float>(w.wcol0 + fn * 16 + r, ks * 4 + kq)];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            a[fm], b[fn], acc[fm][fn], 0, 0, 0);
  }
}

// ---- row-major bf16 fragments the compiler does not fence -----------------
// Same fragments as mfma_compute_tile(bf16), read with asm-issued
// ds_read_b128 for double-buffered loops: before an LDS read it knows of,
// the compiler drains every in-flight LDS-DMA it cannot prove disjoint
// (s_waitcnt vmcnt(0) right after the barrier), which waits for the chunk
// that was issued a few instructions earlier and serialises the loop (see
// tr_frag_issue below for the k-major counterpart). What it cannot see it
// does not wait for, so the caller owns the wait too: issue all fragments
// of a k-step, then rm_frags_wait(). Every fragment read of a chunk has
// then completed before the MFMAs that precede the buffer's freeing barrier.
// An RmFrag holds an asm output register whose data has not landed yet:
// between rm_frag_issue and rm_frags_wait it must not be read, moved or
// copied (keep the fragments in a local array of the issuing function, as
// mfma_compute_tile_nofence does); only get() after the wait is safe.
struct RmFrag {
  s16x8 v;
  DEV bf16x8 get() const { return __builtin_bit_cast(bf16x8, v); }
};

// fragment rows row0..row0+15, k-columns k0..k0+31 of the swizzled
// [rows][BK] image (lds_off)
DEV RmFrag rm_frag_issue(const bf16* img, int row0, int k0, int lane) {
  typedef __attribute__((address_space(3))) const char* lds_p;
  const unsigned base = (unsigned)(size_t)(lds_p)(const char*)img;
  const int off = lds_off<bf16>(row0 + (lane & 15), k0 + (lane >> 4) * 8);
  RmFrag f;
  asm volatile("ds_read_b128 %0, %1"
               : "=v"(f.v) : "v"(base + 2u * (unsigned)off) : "memory");
  return f;
}

// lgkmcnt(0) for the fragments of one k-step; the "+v" operands tie every
// fragment to the wait, so no MFMA that consumes one is scheduled above it
template <int NFM, int NFN>
DEV void rm_frags_wait(RmFrag (&a)[NFM], RmFrag (&b)[NFN]) {
  static_assert(NFM == 4 && (NFN == 2 || NFN == 4), "operand lists below");
  if constexpr (NFN == 2)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0].v), "+v"(a[1].v), "+v"(a[2].v), "+v"(a[3].v),
                   "+v"(b[0].v), "+v"(b[1].v)
                 :: "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0].v), "+v"(a[1].v), "+v"(a[2].v), "+v"(a[3].v),
                   "+v"(b[0].v), "+v"(b[1].v), "+v"(b[2].v), "+v"(b[3].v)
                 :: "memory");
}

// acc += A_tile * B_tile^T-stored: chunk order, k-steps and MFMA sequence of
// mfma_compute_tile(bf16), so the accumulators come out bitwise the same
template <typename S>
DEV void mfma_compute_tile_nofence(const bf16* As, const bf16* Bs,
                                   const WaveCoordT<S>& w,
                                   f32x4 acc[S::FM][S::FN]) {
  constexpr int FM = S::FM, FN = S::FN;
#pragma unroll
  for (int ks = 0; ks < BK / 32; ++ks) {
    RmFrag a[FM], b[FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
      a[fm] = rm_frag_issue(As, w.wrow0 + fm * 16, ks * 32, w.lane);
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      b[fn] = rm_frag_issue(Bs, w.wcol0 + fn * 16, ks * 32, w.lane);
    rm_frags_wait(a, b);
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[fm].get(), b[fn].get(), acc[fm][fn], 0, 0, 0);
  }
}

// ---- hoistable LDS-DMA staging of a [ROWS][BK] image -----------------------
// glds_stage with the lane's slot made explicit: instruction i of the wave
// fills 1 KiB region j = wid*NPW + i, where this lane's 16 bytes are tile
// row glds_row(j, lane), k-columns glds_kk(j, lane) onward. Neither changes
// from chunk to chunk, so callers decode the row once before the k-loop.
template <typename T>
DEV int glds_row(int j, int lane) {
  constexpr int ROWB = BK * (int)sizeof(T);   // bytes per image row
  return (1024 / ROWB) * j + lane / (ROWB / 16);
}
template <typename T>
DEV int glds_kk(int j, int lane) {
  constexpr int LPR = BK * (int)sizeof(T) / 16;   // lanes per row
  const int rl = glds_row<T>(j, lane);
  const int byte = ((lane % LPR) * 16) ^ ((((rl >> 3) ^ rl) & 7) << 4);
  return byte / (int)sizeof(T);                   // lds_off's swizzle
}
// j must be wave-uniform (the DMA's LDS base is a scalar operand)
template <typename T>
DEV void glds_issue(T* img, int j, const T* src) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)src,
      (__attribute__((address_space(3))) unsigned int*)
          &img[j * (1024 / (int)sizeof(T))],
      16, 0, 0);
}

// ---- k-major bf16 images + transposed fragment reads (gfx950) -------------
// A TN product (wgrad: both operands lie k-major in memory, [k][row]) needs
// no transpose on the way INTO LDS: the image keeps the memory layout,
// [BK k-rows][NCH 16-byte chunks], filled by 16B LDS-DMA, and
// ds_read_b64_tr_b16 transposes on the way out -- per 16-lane group it
// fetches a 4 k-row x 16-column block and hands lane i column i, i.e. 4
// k-values of one operand row; two reads make a 16x16x32 fragment's 8.
//
// Bank rule (bank = (addr/4) % 64, conflicts counted per 32-lane half): a
// half's two groups read blocks 8 k-rows apart in the same 16 columns, so
// its 32 lanes (q = k-row in block, b = group, p = 8-byte piece of the 32-byte
// column run) must cover 32 distinct 8-byte slots of a 256-byte bank line.
//   NCH=16 (256-B rows, one bank line per row): slot = 2*(ch^key) + (p&1);
//     key = ((row&3)<<2) | ((row>>2)&3) puts q in chunk bits 2-3 and b (row
//     bit 3) in bit 1, the fragment's p>>1 is bit 0: 16 distinct chunks.
//   NCH=8 (128-B rows, two rows per bank line): slot = 16*(row&1) +
//     2*(ch^key) + (p&1); key = (row&2) | (((row>>3)&1)<<2) puts q>>1 in
//     chunk bit 1 and b in bit 2: 8 distinct chunks in each line half.
using s16x4 = __attribute__((ext_vector_type(4))) short;

template <int NCH>
DEV int kmaj_key(int row) {
  static_assert(NCH == 16 || NCH == 8, "128- or 64-column bf16 image");
  if constexpr (NCH == 16) return ((row & 3) << 2) | ((row >> 2) & 3);
  else return (row & 2) | (((row >> 3) & 1) << 2);
}

// byte offset of 16-byte chunk ch of k-row `row`; the store (DMA source
// swizzle) and every read go through this one function
template <int NCH>
DEV int kmaj_off(int row, int ch) {
  return 16 * NCH * row + 16 * (ch ^ kmaj_key<NCH>(row));
}

// fills a [BK][NCH*8] image: each glds instruction covers a lane-linear
// 1 KiB region, lane -> (k-row, physical chunk), and asks
// addr(i, row, ch) for the LOGICAL chunk that belongs there (16B-aligned
// source or the zero page; no exec masking). i = the wave's instruction
// index, so callers can hoist per-instruction state out of the k-loop: a
// lane's (row-in-tile, ch) never changes from chunk to chunk.
template <int NCH, typename S = TileStd, typename AddrFn>
DEV void glds_stage_kmajor(bf16* img, const WaveCoordT<S>& w, AddrFn&& addr) {
  constexpr int RPK = 64 / NCH;                 // k-rows per 1 KiB region
  constexpr int NPW = BK * NCH * 16 / 1024 / 4;  // regions per wave
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    // the DMA's LDS base is a scalar operand: tell the compiler the wave
    // id is uniform, or it wraps every glds in a waterfall loop
    const int j = __builtin_amdgcn_readfirstlane(w.wid) * NPW + i;
    const int row = RPK * j + w.lane / NCH;
    const int ch = (w.lane % NCH) ^ kmaj_key<NCH>(row);
    const bf16* src = addr(i, row, ch);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)&img[j * 512], 16, 0,
        0);
  }
}
template <int NCH>
constexpr int glds_kmajor_count() { return BK * NCH * 16 / 1024 / 4; }

// 16x16x32 MFMA operand fragment for image columns col0..col0+15 over
// k-rows krow0..krow0+31. Lane group g holds k-rows krow0 + 16*(g>>1) +
// 8*(g&1) + {0..7}: any k order is valid as long as A and B share it.
// EXEC must be all ones here (the gather crosses lanes).
//
// The reads are inline asm, not the ds_read_tr16 builtin: before an LDS
// read it knows of, the compiler drains every in-flight LDS-DMA it cannot
// prove disjoint (s_waitcnt vmcnt(0) -- seen right after the barrier with
// the builtin, even with one LDS object per buffer), which serialises a
// double-buffered k-loop. What it cannot see it does not wait for, so the
// caller owns the wait too: issue all fragments, then tr_frags_wait().
struct TrFrag {
  s16x4 lo, hi;
  DEV bf16x8 get() const {
    s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  }
};

template <int NCH>
DEV TrFrag tr_frag_issue(const bf16* img, int krow0, int col0, int lane) {
  typedef __attribute__((address_space(3))) const char* lds_p;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = krow0 + 16 * (g >> 1) + 8 * (g & 1) + q;
  const int ch = (col0 >> 3) + (p >> 1);
  const unsigned base = (unsigned)(size_t)(lds_p)(const char*)img + 8 * (p & 1);
  TrFrag f;
  asm volatile("ds_read_b64_tr_b16 %0, %1"
               : "=v"(f.lo) : "v"(base + kmaj_off<NCH>(row, ch)) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1"
               : "=v"(f.hi) : "v"(base + kmaj_off<NCH>(row + 4, ch)) : "memory");
  return f;
}

// lgkmcnt(0) for the fragments of one k-step; the "+v" operands tie every
// fragment to the wait, so no MFMA that consumes one is scheduled above it
template <typename S = TileStd>
DEV void tr_frags_wait(TrFrag (&a)[S::FM], TrFrag (&b)[S::FN]) {
  static_assert(S::FM == 4 && (S::FN == 2 || S::FN == 4),
                "operand lists below");
  if constexpr (S::FN == 2)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0].lo), "+v"(a[0].hi), "+v"(a[1].lo), "+v"(a[1].hi),
                   "+v"(a[2].lo), "+v"(a[2].hi), "+v"(a[3].lo), "+v"(a[3].hi),
                   "+v"(b[0].lo), "+v"(b[0].hi), "+v"(b[1].lo), "+v"(b[1].hi)
                 :: "memory");
  else   // 16 tied operands, under the 30 an asm statement may have
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0].lo), "+v"(a[0].hi), "+v"(a[1].lo), "+v"(a[1].hi),
                   "+v"(a[2].lo), "+v"(a[2].hi), "+v"(a[3].lo), "+v"(a[3].hi),
                   "+v"(b[0].lo), "+v"(b[0].hi), "+v"(b[1].lo), "+v"(b[1].hi),
                   "+v"(b[2].lo), "+v"(b[2].hi), "+v"(b[3].lo), "+v"(b[3].hi)
                 :: "memory");
}

// ---- column sums of a transposed B tile Bs[BN][BK] ------------------------
// A conv bias gradient (db[co] = sum_m dy[m][co]) is wgrad with x == 1, and
// the dy tile already sits in LDS as Bs[co][m]. Four threads share a column
// and sum a quarter of its BK values each in fp32 (fixed order, so the sum
// is deterministic); the caller keeps ONE running float per thread. (An
// all-ones MFMA does the same sum but needs an f32x4 accumulator plus two
// fragments: 122 -> 132 VGPR in k_conv_wgrad_vec<bf16>, 4 -> 3 waves/SIMD.)
static_assert(THREADS == 4 * BN, "4 threads per B-tile column");
template <typename T>
DEV float colsum_tile_partial(const T* Bs) {
  constexpr int V = 16 / (int)sizeof(T);
  const int co = threadIdx.x >> 2;
  const int m0 = (threadIdx.x & 3) * (BK / 4);
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < BK / 4; c += V) {
    Pack16<T> v = *(const Pack16<T>*)&Bs[lds_off<T>(co, m0 + c)];
#pragma unroll
    for (int j = 0; j < V; ++j) s += VecIO<T>::to_f32(v.e[j]);
  }
  return s;
}

// folds the four per-thread partials of a column; valid where
// (threadIdx.x & 3) == 0, for tile column threadIdx.x >> 2
DEV float colsum_tile_finish(float s) {
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  return s;
}

// ---- epilogue: C/D fragment map col=lane&15, row=(lane>>4)*4+j ------------
// Visits every accumulator element with its global (row, col).
template <typename S, typename F>
DEV void epilogue_visit(const WaveCoordT<S>& w, f32x4 acc[S::FM][S::FN],
                        int row0, int col0, F&& emit) {
  constexpr int FM = S::FM, FN = S::FN;
  const int cr = (w.lane >> 4) * 4;
  const int cc = w.lane & 15;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int row = row0 + w.wrow0 + fm * 16 + cr + j;
        int col = col0 + w.wcol0 + fn * 16 + cc;
        emit(row, col, acc[fm][fn][j]);
      }
}

}  // namespace tile
