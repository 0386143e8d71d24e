// On-device sampling from bf16 logits: temperature, top-k, top-p and the
// draw in one kernel, one 1024-thread workgroup per row (a 50,257-entry
// bf16 row is 100 KB and stays in L2 across the passes). The step counter
// is a device int64, so a captured decode graph draws fresh numbers on
// every replay.
//
// Semantics (ops/functional.py::sample_logits is the same rules in torch):
//   z_i = float(logit_i) / temperature; temperature == 0 or top_k == 1 is
//   greedy (lowest index among the maxima).
//   top-k keeps {z_i >= t_k}, t_k the k-th largest value, ties included.
//   top-p keeps {z_i >= t_p}, t_p the largest value whose tail mass
//   (renormalised over the top-k survivors) reaches top_p, ties included.
//   The draw returns the first kept index, in token order, whose running
//   sum of exp(z_i - max) reaches u * total, u in (0, 1].
//
// The result is a pure function of the inputs. bf16 logits have 16-bit
// order-preserving keys, so two 8-bit histogram passes give each exact
// threshold. Probability mass is accumulated as 64-bit fixed point
// (exp(z - max) * 2^40, integer adds): integer sums are associative, so
// neither the LDS atomics of the histograms nor the block scan of the
// draw depend on execution order.

#include "common.h"
#include "kernels.h"

namespace tnn {

namespace {

using u64 = unsigned long long;
constexpr int ST = 1024;
constexpr float FX_ONE = 1099511627776.0f;  // 2^40

// order-preserving 16-bit key of a bf16 bit pattern (-0 folded onto +0)
DEV unsigned key_of(unsigned short b) {
  if ((b & 0x7FFF) == 0) b = 0;
  return (b & 0x8000) ? (unsigned)(~b & 0xFFFF) : (unsigned)(b | 0x8000);
}

DEV float val_of_key(unsigned k) {
  const unsigned b = (k & 0x8000) ? (k & 0x7FFF) : (~k & 0xFFFF);
  return __uint_as_float(b << 16);
}

DEV u64 mass_fx(unsigned k, float temperature, float zmax) {
  return (u64)(__expf(val_of_key(k) / temperature - zmax) * FX_ONE);
}

// Given hist[256], find the largest bin b whose suffix sum
// S(b) = sum_{j >= b} hist[j] reaches the target (bin 0 if none does).
// frac > 0: target = max(1, ceil(frac * S(0))), else the given target.
// Returns b; `above` = S(b + 1), `target` = the target used. All threads
// of the block must call it.
DEV unsigned suffix_find(const u64* hist, u64* scan, u64* res, double frac,
                         u64& target, u64& above) {
  const int t = threadIdx.x;
  if (t < 256) scan[t] = hist[t];
  for (int off = 1; off < 256; off <<= 1) {
    __syncthreads();
    const u64 v = (t < 256 && t + off < 256) ? scan[t + off] : 0;
    __syncthreads();
    if (t < 256) scan[t] += v;
  }
  __syncthreads();
  if (frac > 0.0) {
    const u64 tot = scan[0];
    u64 tg = (u64)ceil(frac * (double)tot);
    if (tg > tot) tg = tot;
    target = tg < 1 ? 1 : tg;
  }
  if (t < 256) {
    const u64 nxt = t == 255 ? 0 : scan[t + 1];
    if ((t == 0 || scan[t] >= target) && (t == 255 || nxt < target)) {
      res[0] = (u64)t;
      res[1] = nxt;
    }
  }
  __syncthreads();
  const unsigned b = (unsigned)res[0];
  above = res[1];
  __syncthreads();
  return b;
}

__launch_bounds__(ST)
__global__ void k_sample_logits(const unsigned short* __restrict__ logits,
                                int64_t* __restrict__ ids, int V,
                                float temperature, int top_k, float top_p,
                                u64 seed, const int64_t* __restrict__ step,
                                const float* __restrict__ u_in) {
  __shared__ u64 hist[256];
  __shared__ u64 scan[256];
  __shared__ u64 res[2];
  __shared__ u64 best;
  __shared__ u64 sums[ST];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const unsigned short* lr = logits + (int64_t)row * V;

  // maximum key, lowest index among its occurrences: one 64-bit max over
  // (key << 32 | ~index)
  if (tid == 0) best = 0;
  __syncthreads();
  u64 b = 0;
  for (int i = tid; i < V; i += ST) {
    const u64 c = ((u64)key_of(lr[i]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
    b = c > b ? c : b;
  }
  atomicMax(&best, b);
  __syncthreads();
  const unsigned kmax = (unsigned)(best >> 32);
  const int imax = (int)(0xFFFFFFFFu - (unsigned)best);
  if (temperature == 0.0f || top_k == 1) {
    if (tid == 0) ids[row] = imax;
    return;
  }

  // ---- top-k: exact k-th largest key by two 8-bit histogram passes --------
  unsigned thr = 0;  // keep keys >= thr
  if (top_k > 0 && top_k < V) {
    u64 target = (u64)top_k, above;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += ST)
      atomicAdd(&hist[key_of(lr[i]) >> 8], (u64)1);
    __syncthreads();
    const unsigned hb = suffix_find(hist, scan, res, 0.0, target, above);
    target -= above;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += ST) {
      const unsigned k = key_of(lr[i]);
      if ((k >> 8) == hb) atomicAdd(&hist[k & 255], (u64)1);
    }
    __syncthreads();
    const unsigned lb = suffix_find(hist, scan, res, 0.0, target, above);
    thr = (hb << 8) | lb;
  }

  const float zmax = val_of_key(kmax) / temperature;

  // ---- top-p over the survivors: the same two passes on fixed-point mass --
  if (top_p < 1.0f) {
    u64 target = 0, above;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += ST) {
      const unsigned k = key_of(lr[i]);
      if (k >= thr) atomicAdd(&hist[k >> 8], mass_fx(k, temperature, zmax));
    }
    __syncthreads();
    const unsigned hb =
        suffix_find(hist, scan, res, (double)top_p, target, above);
    target -= above;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += ST) {
      const unsigned k = key_of(lr[i]);
      if (k >= thr && (k >> 8) == hb)
        atomicAdd(&hist[k & 255], mass_fx(k, temperature, zmax));
    }
    __syncthreads();
    const unsigned lb = suffix_find(hist, scan, res, 0.0, target, above);
    const unsigned thr_p = (hb << 8) | lb;
    thr = thr_p > thr ? thr_p : thr;
  }

  // ---- draw: token-order running sum over contiguous per-thread chunks ----
  const int chunk = (V + ST - 1) / ST;
  const int lo = min(V, tid * chunk), hi = min(V, lo + chunk);
  u64 s = 0;
  for (int i = lo; i < hi; ++i) {
    const unsigned k = key_of(lr[i]);
    if (k >= thr) s += mass_fx(k, temperature, zmax);
  }
  sums[tid] = s;
  for (int off = 1; off < ST; off <<= 1) {
    __syncthreads();
    const u64 v = tid >= off ? sums[tid - off] : 0;
    __syncthreads();
    sums[tid] += v;
  }
  __syncthreads();
  const u64 total = sums[ST - 1];  // >= 2^40: the maximum is always kept
  float u;
  if (u_in) {
    u = u_in[row];
  } else {
    const Philox rng(seed);
    u = u32_to_uniform(rng(((u64)step[0] << 32) | (u64)(unsigned)row).x);
  }
  u64 target = (u64)ceil((double)u * (double)total);
  target = target < 1 ? 1 : (target > total ? total : target);
  // 1 <= target <= total, so exactly one chunk's (excl, incl] holds it;
  // the maximum's index stands in should that ever fail
  if (tid == 0) ids[row] = imax;
  __syncthreads();
  const u64 incl = sums[tid], excl = incl - s;
  if (excl < target && incl >= target) {
    u64 run = excl;
    for (int i = lo; i < hi; ++i) {
      const unsigned k = key_of(lr[i]);
      if (k < thr) continue;
      run += mass_fx(k, temperature, zmax);
      if (run >= target) {
        ids[row] = i;
        break;
      }
    }
  }
}

}  // namespace

void sample_logits_launch(const void* logits, int64_t* ids, int R, int V,
                          float temperature, int top_k, float top_p,
                          uint64_t seed, const int64_t* step, const float* u,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_sample_logits, dim3(R), dim3(ST), 0, s,
                     (const unsigned short*)logits, ids, V, temperature, top_k,
                     top_p, (u64)seed, step, u);
}

}  // namespace tnn
