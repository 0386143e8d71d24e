// Torch bindings for the tnn_amd gfx950 kernels.
//
// Tensor-level checks live here; the .hip translation units only see raw
// pointers + shapes + the stream. Every entry point CHECKs device/layout —
// a CPU tensor reaching these is a dispatch bug in the python layer.

#include <array>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "kernels.h"

namespace tnn {

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// 16-byte zero page for glds source redirection (invalid lanes load
// zeros instead of being exec-masked, which would leave stale LDS)
static void* zero_page(const at::Tensor& like) {
  static at::Tensor z;
  if (!z.defined() || z.device() != like.device())
    z = at::zeros({16}, like.options().dtype(at::kFloat));
  return z.data_ptr();
}

static DT dt_of(const at::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return DT::F32;
  if (t.scalar_type() == at::kBFloat16) return DT::BF16;
  TORCH_CHECK(false, "tnn_amd kernels support fp32/bf16, got ", t.scalar_type());
}

#define CHECK_IN(t)                                             \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");             \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// The GEMM entry points raise on an empty operand instead of launching a
// zero-sized grid (an invalid launch) or returning an epilogue of nothing.
#define CHECK_NONEMPTY(fn, M, N, K)                                   \
  TORCH_CHECK((M) >= 1 && (N) >= 1 && (K) >= 1, fn ": empty operand", \
              " (M = ", (M), ", N = ", (N), ", K = ", (K), ")")

// ---- elementwise -----------------------------------------------------------
at::Tensor act_fwd(const at::Tensor& x, int64_t kind) {
  CHECK_IN(x);
  auto y = at::empty_like(x);
  act_fwd_launch(dt_of(x), x.data_ptr(), y.data_ptr(), x.numel(), (int)kind,
                 cur_stream());
  return y;
}

at::Tensor act_bwd(const at::Tensor& dy, const at::Tensor& x,
                   const at::Tensor& y, int64_t kind) {
  CHECK_IN(dy);
  auto dx = at::empty_like(dy);
  act_bwd_launch(dt_of(dy), dy.data_ptr(), x.data_ptr(), y.data_ptr(),
                 dx.data_ptr(), dy.numel(), (int)kind, cur_stream());
  return dx;
}

at::Tensor add_act_fwd(const at::Tensor& a, const at::Tensor& b,
                       int64_t kind) {
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.sizes() == b.sizes() && a.scalar_type() == b.scalar_type());
  auto y = at::empty_like(a);
  add_act_fwd_launch(dt_of(a), a.data_ptr(), b.data_ptr(), y.data_ptr(),
                     a.numel(), (int)kind, cur_stream());
  return y;
}

at::Tensor add_act_bwd(const at::Tensor& dy, const at::Tensor& y,
                       int64_t kind) {
  CHECK_IN(dy);
  auto g = at::empty_like(dy);
  add_act_bwd_launch(dt_of(dy), dy.data_ptr(), y.data_ptr(), g.data_ptr(),
                     dy.numel(), (int)kind, cur_stream());
  return g;
}

at::Tensor relu_bwd_mask(const at::Tensor& dy, const at::Tensor& y) {
  CHECK_IN(dy);
  CHECK_IN(y);
  auto dx = at::empty_like(dy);
  relu_bwd_mask_launch(dt_of(dy), dy.data_ptr(), y.data_ptr(), dx.data_ptr(),
                       dy.numel(), cur_stream());
  return dx;
}

std::vector<at::Tensor> dropout_fwd(const at::Tensor& x, double p,
                                    int64_t seed,
                                    const c10::optional<at::Tensor>& ctr) {
  CHECK_IN(x);
  auto y = at::empty_like(x);
  auto mask = at::empty(x.sizes(), x.options().dtype(at::kByte));
  const int64_t* ctrp = ctr.has_value() ? ctr->data_ptr<int64_t>() : nullptr;
  dropout_fwd_launch(dt_of(x), x.data_ptr(), y.data_ptr(),
                     mask.data_ptr<uint8_t>(), x.numel(), (float)p,
                     (uint64_t)seed, ctrp, cur_stream());
  return {y, mask};
}

at::Tensor dropout_bwd(const at::Tensor& dy, const at::Tensor& mask, double p) {
  CHECK_IN(dy);
  auto dx = at::empty_like(dy);
  dropout_bwd_launch(dt_of(dy), dy.data_ptr(), mask.data_ptr<uint8_t>(),
                     dx.data_ptr(), dy.numel(), (float)p, cur_stream());
  return dx;
}

at::Tensor colsum(const at::Tensor& x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 2, "colsum wants [rows, cols]");
  const int slices = colsum_ws_slices(dt_of(x), x.data_ptr(), x.size(0),
                                      x.size(1));
  // vec path writes per-slice slabs + a finalize (no zero-init needed);
  // scalar fallback atomically accumulates into a zeroed output
  auto out = slices >= 1
                 ? at::empty({x.size(1)}, x.options().dtype(at::kFloat))
                 : at::zeros({x.size(1)}, x.options().dtype(at::kFloat));
  at::Tensor ws;
  float* wp = nullptr;
  if (slices > 1) {
    ws = at::empty({(int64_t)slices * x.size(1)},
                   x.options().dtype(at::kFloat));
    wp = ws.data_ptr<float>();
  }
  colsum_launch(dt_of(x), x.data_ptr(), out.data_ptr(), wp, slices, x.size(0),
                x.size(1), cur_stream());
  if (x.scalar_type() != at::kFloat) {
    auto out_t = at::empty({x.size(1)}, x.options());
    cast_f32_launch(dt_of(x), out.data_ptr<float>(), out_t.data_ptr(),
                    out.numel(), cur_stream());
    return out_t;
  }
  return out;
}

// ---- gemm ------------------------------------------------------------------
// TNN_GEMM32=0 sends bf16 NT shapes to the 16x16-MFMA kernels instead of
// the 32x32 one (read once per process)
static bool gemm32_enabled() {
  static const bool on = [] {
    const char* e = getenv("TNN_GEMM32");
    return !(e && e[0] == '0');
  }();
  return on;
}

// fp32 split-K slabs [z, rows*cols]; none (null) when unsplit
static float* splitk_ws(at::Tensor& ws, const at::Tensor& like, int z,
                        int64_t rows, int64_t cols, bool force = false) {
  if (z <= 1 && !force) return nullptr;
  ws = at::empty({(int64_t)z * rows * cols}, like.options().dtype(at::kFloat));
  return ws.data_ptr<float>();
}

at::Tensor gemm(const at::Tensor& a, const at::Tensor& b,
                const c10::optional<at::Tensor>& bias, int64_t act_kind,
                const c10::optional<at::Tensor>& residual = c10::nullopt,
                const c10::optional<at::Tensor>& ln_gamma = c10::nullopt,
                const c10::optional<at::Tensor>& ln_beta = c10::nullopt,
                double ln_eps = 1e-5) {
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(0),
              "gemm shapes ", a.sizes(), " @ ", b.sizes());
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "gemm dtype mismatch ",
              a.scalar_type(), " vs ", b.scalar_type());
  int M = a.size(0), K = a.size(1), N = b.size(1);
  CHECK_NONEMPTY("gemm", M, N, K);
  auto c = at::empty({M, N}, a.options());
  const void* bp = nullptr;
  if (bias.has_value()) {
    // the kernels read bias as a's element type, N entries
    TORCH_CHECK(bias->is_cuda(), "gemm bias must be on GPU");
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N &&
                bias->scalar_type() == a.scalar_type(),
                "gemm bias must be contiguous [", N, "] ", a.scalar_type(),
                ", got ", bias->sizes(), " ", bias->scalar_type());
    bp = bias->data_ptr();
  }
  const void* rp = nullptr;
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_cuda(), "gemm residual must be on GPU");
    TORCH_CHECK(residual->is_contiguous() &&
                residual->scalar_type() == a.scalar_type() &&
                residual->numel() == (int64_t)M * N,
                "gemm residual mismatch");
    rp = residual->data_ptr();
  }
  const float* lng = nullptr;
  const float* lnb = nullptr;
  if (ln_gamma.has_value()) {
    TORCH_CHECK(M == 1 && K <= GEMV1_MAX_K && ln_beta.has_value() &&
                ln_gamma->scalar_type() == at::kFloat &&
                ln_beta->scalar_type() == at::kFloat,
                "fused ln: decode GEMV only, fp32 gamma/beta");
    // the kernel reads K floats from each, on the device
    TORCH_CHECK(ln_gamma->is_cuda() && ln_gamma->is_contiguous() &&
                ln_gamma->numel() == K,
                "gemm ln_gamma must be a contiguous GPU tensor of [", K,
                "], got ", ln_gamma->sizes(), " on ", ln_gamma->device());
    TORCH_CHECK(ln_beta->is_cuda() && ln_beta->is_contiguous() &&
                ln_beta->numel() == K,
                "gemm ln_beta must be a contiguous GPU tensor of [", K,
                "], got ", ln_beta->sizes(), " on ", ln_beta->device());
    lng = ln_gamma->data_ptr<float>();
    lnb = ln_beta->data_ptr<float>();
  }
  if (M == 1) {
    if (K <= GEMV1_MAX_K) {
      // LDS-cached matvec; K-split across blocks to fill the chip (fp32
      // partials + a parallel finalize) when N alone is too narrow
      int ns = gemv_nn1_nsplit(N, K);
      at::Tensor part;
      float* pp = splitk_ws(part, a, ns, 1, N);
      gemv_nn1_launch(dt_of(a), a.data_ptr(), b.data_ptr(), bp, rp,
                      c.data_ptr(), pp, ns, lng, lnb, (float)ln_eps, N, K,
                      (int)act_kind, cur_stream());
      return c;
    }
    // huge-K fallback: K-split partials + finalize (no residual fusion)
    TORCH_CHECK(rp == nullptr, "gemm residual unsupported for K > 8192 M=1");
    int ks = gemv_nn_ksplits(N, K);
    auto ws = at::empty({(int64_t)ks * N}, a.options().dtype(at::kFloat));
    gemv_nn_launch(dt_of(a), a.data_ptr(), b.data_ptr(), bp, c.data_ptr(),
                   ws.data_ptr<float>(), ks, N, K, (int)act_kind,
                   cur_stream());
    return c;
  }
  bool vec_ok = (dt_of(a) == DT::F32 ? K % 4 == 0 : K % 8 == 0) &&
                ptr_aligned16(a.data_ptr());
  if (M >= 64 && vec_ok) {
    // transpose the (weight-sized) B once and take the NT glds path: B rows
    // become k-contiguous LDS-DMA targets instead of a VGPR scatter
    auto bt = at::empty({(int64_t)N, (int64_t)K}, b.options());
    transpose_w_launch(dt_of(b), b.data_ptr(), bt.data_ptr(), 1, 1, K, N,
                       cur_stream());
    at::Tensor ws;
    if (gemm32_enabled() && dt_of(a) == DT::BF16) {
      // 32x32x16-MFMA tile core (peak issue at this kernel's 2
      // waves/SIMD residency; the 16x16x32 core needs 3-4)
      int z = N % 4 == 0 ? gemm_nt32_zsplits(M, N, K) : 1;
      gemm_nt32_launch(a.data_ptr(), bt.data_ptr(), splitk_ws(ws, a, z, M, N),
                       bp, rp, c.data_ptr(), z, zero_page(a), M, N, K,
                       (int)act_kind, cur_stream());
      return c;
    }
    const int zf = N % 4 == 0 ? gemm_nt_fsplits(dt_of(a), M, N, K) : 1;
    if (zf > 1 && K <= 3072 && ptr_aligned16(bt.data_ptr())) {
      gemm_nt_zf_launch(dt_of(a), a.data_ptr(), bt.data_ptr(),
                        splitk_ws(ws, a, zf, M, N), bp, rp, c.data_ptr(), zf,
                        zero_page(a), M, N, K, (int)act_kind, cur_stream());
      return c;
    }
    gemm_launch(dt_of(a), a.data_ptr(), bt.data_ptr(), bp, c.data_ptr(),
                zero_page(a), rp, M, N, K, /*trans_b=*/true, (int)act_kind,
                cur_stream());
    return c;
  }
  gemm_launch(dt_of(a), a.data_ptr(), b.data_ptr(), bp, c.data_ptr(),
              zero_page(a), rp, M, N, K, /*trans_b=*/false, (int)act_kind,
              cur_stream());
  return c;
}

// TNN_SKINNY=0 keeps ops.linear off the skinny route (A/B timing and an
// escape hatch; read once per process)
static bool skinny_enabled() {
  static const bool on = [] {
    const char* e = getenv("TNN_SKINNY");
    return !(e && e[0] == '0');
  }();
  return on;
}

// y[M,N] = act(LN?(a)[M,K] @ b[K,N] + bias) + residual for M <= 16
// (batched decode): every weight element is read once for all M rows.
// A separate entry point, so ext.gemm keeps its numerics at tiny M.
at::Tensor gemm_skinny(const at::Tensor& a, const at::Tensor& b,
                       const c10::optional<at::Tensor>& bias, int64_t act_kind,
                       const c10::optional<at::Tensor>& residual,
                       const c10::optional<at::Tensor>& ln_gamma,
                       const c10::optional<at::Tensor>& ln_beta,
                       double ln_eps) {
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(0),
              "gemm_skinny shapes ", a.sizes(), " @ ", b.sizes());
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "gemm_skinny dtype mismatch ",
              a.scalar_type(), " vs ", b.scalar_type());
  const DT dt = dt_of(a);  // fp32 / bf16 only
  const int M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(M >= 1 && M <= SKINNY_MAX_M, "gemm_skinny wants 1 <= M <= ",
              SKINNY_MAX_M, ", got M = ", M);
  CHECK_NONEMPTY("gemm_skinny", M, N, K);
  auto c = at::empty({M, N}, a.options());
  const void* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                bias->numel() == N && bias->scalar_type() == a.scalar_type(),
                "gemm_skinny bias must be contiguous [", N, "] ",
                a.scalar_type());
    bp = bias->data_ptr();
  }
  const void* rp = nullptr;
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() &&
                residual->scalar_type() == a.scalar_type() &&
                residual->numel() == (int64_t)M * N,
                "gemm_skinny residual mismatch");
    rp = residual->data_ptr();
  }
  const float* lng = nullptr;
  const float* lnb = nullptr;
  if (ln_gamma.has_value()) {
    TORCH_CHECK(ln_beta.has_value() && ln_gamma->is_cuda() &&
                ln_beta->is_cuda() && ln_gamma->is_contiguous() &&
                ln_beta->is_contiguous() &&
                ln_gamma->scalar_type() == at::kFloat &&
                ln_beta->scalar_type() == at::kFloat &&
                ln_gamma->numel() == K && ln_beta->numel() == K,
                "fused ln wants contiguous fp32 gamma/beta [", K, "]");
    lng = ln_gamma->data_ptr<float>();
    lnb = ln_beta->data_ptr<float>();
  }
  const int ns = gemm_skinny_nsplit(dt, M, N, K);
  at::Tensor part;
  float* pp = splitk_ws(part, a, ns, M, N);
  gemm_skinny_launch(dt, a.data_ptr(), b.data_ptr(), bp, rp, c.data_ptr(), pp,
                     ns, lng, lnb, (float)ln_eps, M, N, K, (int)act_kind,
                     cur_stream());
  return c;
}

at::Tensor gemm_nt(const at::Tensor& a, const at::Tensor& b) {
  // c[m, j] = sum_k a[m, k] * b[j, k]
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1),
              "gemm_nt shapes ", a.sizes(), " @ ", b.sizes(), "^T");
  // both operands are read as a's element type
  TORCH_CHECK(a.scalar_type() == b.scalar_type(),
              "gemm_nt dtype mismatch: b is ", b.scalar_type(), ", a is ",
              a.scalar_type());
  int M = a.size(0), K = a.size(1), N = b.size(0);
  CHECK_NONEMPTY("gemm_nt", M, N, K);
  auto c = at::empty({M, N}, a.options());
  at::Tensor ws;
  if (gemm32_enabled() && dt_of(a) == DT::BF16 && K % 8 == 0 &&
      ptr_aligned16(a.data_ptr()) && ptr_aligned16(b.data_ptr())) {
    int z32 = N % 4 == 0 ? gemm_nt32_zsplits(M, N, K) : 1;
    gemm_nt32_launch(a.data_ptr(), b.data_ptr(), splitk_ws(ws, a, z32, M, N),
                     /*bias=*/nullptr, /*resid=*/nullptr, c.data_ptr(), z32,
                     zero_page(a), M, N, K, 0, cur_stream());
    return c;
  }
  int z = gemm_nt_zsplits(dt_of(a), M, N, K);
  if (z > 1 && ptr_aligned16(a.data_ptr()) && ptr_aligned16(b.data_ptr())) {
    // huge-K underfilled shape (vocab-head dgrad): K-split fp32 slabs
    gemm_nt_z_launch(dt_of(a), a.data_ptr(), b.data_ptr(),
                     splitk_ws(ws, a, z, M, N), c.data_ptr(), dt_of(a), z,
                     zero_page(a), M, N, K, cur_stream());
    return c;
  }
  gemm_launch(dt_of(a), a.data_ptr(), b.data_ptr(), nullptr, c.data_ptr(),
              zero_page(a), /*resid=*/nullptr, M, N, K, /*trans_b=*/true, 0,
              cur_stream());
  return c;
}

at::Tensor gemm_tn(const at::Tensor& a, const at::Tensor& b, bool out_in_dt) {
  // c[k, n] = sum_m a[m, k] * b[m, n]  (fp32 accumulate; output fp32, or
  // a's dtype when out_in_dt -- the cast rides the split-K reduce)
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(0) == b.size(0),
              "gemm_tn shapes ", a.sizes(), "^T @ ", b.sizes());
  TORCH_CHECK(a.scalar_type() == b.scalar_type(),
              "gemm_tn dtype mismatch: b is ", b.scalar_type(), ", a is ",
              a.scalar_type());
  int M = a.size(0), K = a.size(1), N = b.size(1);
  CHECK_NONEMPTY("gemm_tn", M, N, K);
  DT out_dt = out_in_dt ? dt_of(a) : DT::F32;
  auto c = at::empty({K, N}, out_dt == DT::F32
                                 ? a.options().dtype(at::kFloat)
                                 : a.options());
  int z = gemm_tn_zsplits(M, N, K);
  at::Tensor ws;
  // a cast output goes through the reduce (and so a slab) even unsplit
  float* wsp = splitk_ws(ws, a, z, K, N, /*force=*/out_dt != DT::F32);
  gemm_tn_launch(dt_of(a), a.data_ptr(), b.data_ptr(), c.data_ptr(), out_dt,
                 wsp, z, zero_page(a), M, N, K, cur_stream());
  return c;
}

at::Tensor mfma_selftest(const at::Tensor& a, const at::Tensor& b) {
  // a: [16, 32] bf16, b: [32, 16] bf16 -> d [16, 16] f32 (layout check)
  CHECK_IN(a);
  auto d = at::zeros({16, 16}, a.options().dtype(at::kFloat));
  mfma_selftest_launch(a.data_ptr(), b.data_ptr(), d.data_ptr<float>(),
                       cur_stream());
  return d;
}

at::Tensor mfma_selftest_f32(const at::Tensor& a, const at::Tensor& b) {
  // a: [16, 4] f32, b: [4, 16] f32 -> d [16, 16] f32
  CHECK_IN(a);
  auto d = at::zeros({16, 16}, a.options().dtype(at::kFloat));
  mfma_selftest_f32_launch(a.data_ptr<float>(), b.data_ptr<float>(),
                           d.data_ptr<float>(), cur_stream());
  return d;
}

// ---- conv2d ----------------------------------------------------------------
// The kernels take one ConvShape and trust it, so every entry point and its
// *_route twin builds it here, and everything below raises before any launch.
// shape of the conv whose input is [N, H, W, Cin] and output [N, OH, OW, Cout]
static ConvShape conv_shape_out(const char* fn, int64_t N, int64_t H,
                                int64_t W, int64_t Cin, int64_t Cout,
                                int64_t KH, int64_t KW, int64_t SH, int64_t SW,
                                int64_t PH, int64_t PW, int64_t OH,
                                int64_t OW) {
  TORCH_CHECK(SH >= 1 && SW >= 1, fn, ": stride must be >= 1, got (", SH,
              ", ", SW, ")");
  TORCH_CHECK(PH >= 0 && PW >= 0, fn, ": padding must be >= 0, got (", PH,
              ", ", PW, ")");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 &&
                  KH >= 1 && KW >= 1,
              fn, ": empty operand (N = ", N, ", H = ", H, ", W = ", W,
              ", Cin = ", Cin, ", Cout = ", Cout, ", KH = ", KH, ", KW = ", KW,
              ")");
  TORCH_CHECK(OH >= 1 && OW >= 1, fn, ": no output pixel (OH = ", OH,
              ", OW = ", OW, ")");
  ConvShape cs;
  cs.N = N;
  cs.H = H;
  cs.W = W;
  cs.Cin = Cin;
  cs.Cout = Cout;
  cs.KH = KH;
  cs.KW = KW;
  cs.SH = SH;
  cs.SW = SW;
  cs.PH = PH;
  cs.PW = PW;
  cs.OH = OH;
  cs.OW = OW;
  cs.init_fdiv();
  return cs;
}

// output extent of one axis; 0 where the padded input is shorter than the
// kernel (C++ division would round -1 / 2 up to 0) or the stride is invalid
static int64_t conv_out_extent(int64_t in, int64_t k, int64_t s, int64_t p) {
  return s >= 1 && in + 2 * p >= k ? (in + 2 * p - k) / s + 1 : 0;
}

static ConvShape conv_shape(const char* fn, const at::Tensor& x, int64_t Cin,
                            int64_t Cout, int64_t KH, int64_t KW, int64_t SH,
                            int64_t SW, int64_t PH, int64_t PW) {
  int64_t H = x.size(1), W = x.size(2);
  return conv_shape_out(fn, x.size(0), H, W, Cin, Cout, KH, KW, SH, SW, PH, PW,
                        conv_out_extent(H, KH, SH, PH),
                        conv_out_extent(W, KW, SW, PW));
}

// operand checks and shape of conv2d_fwd / conv2d_fwd_stats / conv2d_fwd_route
static ConvShape conv_fwd_shape(const char* fn, const at::Tensor& x,
                                const at::Tensor& w, int64_t sh, int64_t sw,
                                int64_t ph, int64_t pw) {
  CHECK_IN(x);
  CHECK_IN(w);
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && x.size(3) == w.size(2), fn,
              " x ", x.sizes(), " w ", w.sizes());
  TORCH_CHECK(x.scalar_type() == w.scalar_type(), fn, " dtype mismatch ",
              x.scalar_type(), " vs ", w.scalar_type());
  return conv_shape(fn, x, w.size(2), w.size(3), w.size(0), w.size(1), sh, sw,
                    ph, pw);
}

// ... of conv2d_dgrad / conv2d_dgrad_route: dy's extents are those the conv
// gives for (H, W), not whatever dy happens to have
static ConvShape conv_dgrad_shape(const char* fn, const at::Tensor& dy,
                                  const at::Tensor& w, int64_t H, int64_t W,
                                  int64_t sh, int64_t sw, int64_t ph,
                                  int64_t pw) {
  CHECK_IN(dy);
  CHECK_IN(w);
  TORCH_CHECK(dy.dim() == 4 && w.dim() == 4, fn, " dy ", dy.sizes(), " w ",
              w.sizes());
  TORCH_CHECK(dy.scalar_type() == w.scalar_type(), fn,
              " dtype mismatch: dy is ", dy.scalar_type(), ", w is ",
              w.scalar_type());
  TORCH_CHECK(dy.size(3) == w.size(3), fn, " dy ", dy.sizes(),
              " has other channels than w ", w.sizes());
  const int64_t KH = w.size(0), KW = w.size(1);
  auto cs = conv_shape_out(fn, dy.size(0), H, W, w.size(2), w.size(3), KH, KW,
                           sh, sw, ph, pw, conv_out_extent(H, KH, sh, ph),
                           conv_out_extent(W, KW, sw, pw));
  TORCH_CHECK(dy.size(1) == cs.OH && dy.size(2) == cs.OW, fn, " dy ",
              dy.sizes(), " is not the output of a ", H, " x ", W,
              " input: expected OH = ", cs.OH, ", OW = ", cs.OW);
  return cs;
}

// ... of conv2d_wgrad / conv2d_wgrad_bias / conv2d_wgrad_route
static ConvShape conv_wgrad_shape(const char* fn, const at::Tensor& x,
                                  const at::Tensor& dy, int64_t KH, int64_t KW,
                                  int64_t sh, int64_t sw, int64_t ph,
                                  int64_t pw) {
  CHECK_IN(x);
  CHECK_IN(dy);
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, fn, " x ", x.sizes(), " dy ",
              dy.sizes());
  TORCH_CHECK(x.scalar_type() == dy.scalar_type(), fn,
              " dtype mismatch: x is ", x.scalar_type(), ", dy is ",
              dy.scalar_type());
  TORCH_CHECK(x.size(0) == dy.size(0), fn, " batch mismatch: x ", x.sizes(),
              " dy ", dy.sizes());
  auto cs = conv_shape(fn, x, x.size(3), dy.size(3), KH, KW, sh, sw, ph, pw);
  TORCH_CHECK(dy.size(1) == cs.OH && dy.size(2) == cs.OW, "wgrad shape");
  return cs;
}

// Returns {y, stats}. want_stats asks for the fused per-channel sum/sumsq of
// y (linear act) as slab partials [m-tiles, 2, Cout], one row per 128-row
// m-tile, written with plain stores into an at::empty tensor (no atomics, no
// zero-init; a fold sums the rows). It comes from the DMA-staged kernels only
// (k_conv_fwd_db / k_conv_fwd_sb), so where those are not eligible (non-pow2
// dims, unaligned x, fp32 with K > 2304, TNN_FWD_DB=0) stats is EMPTY and y
// is computed by the plain route all the same.
static std::vector<at::Tensor> conv2d_fwd_impl(
    const at::Tensor& x, const at::Tensor& w,
    const c10::optional<at::Tensor>& bias, int64_t sh, int64_t sw, int64_t ph,
    int64_t pw, bool relu, bool want_stats) {
  auto cs = conv_fwd_shape("conv2d_fwd", x, w, sh, sw, ph, pw);
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == x.scalar_type(),
                "conv2d bias dtype mismatch");
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                    bias->numel() == cs.Cout,
                "conv2d_fwd: bias must be a contiguous GPU tensor of ",
                cs.Cout, " elements, got ", bias->sizes());
  }
  auto y = at::empty({cs.N, cs.OH, cs.OW, cs.Cout}, x.options());
  at::Tensor wt2, stats;
  const bool db = conv2d_fwd_wants_db(dt_of(x), x.data_ptr(), cs);
  if (db) {
    wt2 = at::empty({(int64_t)cs.Cout, (int64_t)cs.KH * cs.KW * cs.Cin},
                    w.options());
    transpose_w_fwd_launch(dt_of(x), w.data_ptr(), wt2.data_ptr(),
                           cs.KH * cs.KW, cs.Cin, cs.Cout, cur_stream());
  }
  if (want_stats)
    stats = db ? at::empty({(int64_t)conv2d_fwd_stats_rows(cs), 2,
                            (int64_t)cs.Cout},
                           x.options().dtype(at::kFloat))
               : at::empty({0}, x.options().dtype(at::kFloat));
  conv2d_fwd_launch(dt_of(x), x.data_ptr(), w.data_ptr(),
                    db ? wt2.data_ptr() : nullptr,
                    bias.has_value() ? bias->data_ptr() : nullptr,
                    y.data_ptr(), zero_page(x),
                    db && want_stats ? stats.data_ptr<float>() : nullptr, cs,
                    relu, cur_stream());
  return {y, stats};
}

at::Tensor conv2d_fwd(const at::Tensor& x, const at::Tensor& w,
                      const c10::optional<at::Tensor>& bias, int64_t sh,
                      int64_t sw, int64_t ph, int64_t pw, bool relu) {
  return conv2d_fwd_impl(x, w, bias, sh, sw, ph, pw, relu, false)[0];
}

// conv fwd + fused per-channel sum/sumsq for a following train-mode BN
// (linear act). Returns {y, stats[2, Cout]}; callers fall back to the
// separate BN stats pass when stats comes back empty.
std::vector<at::Tensor> conv2d_fwd_stats(const at::Tensor& x,
                                         const at::Tensor& w,
                                         const c10::optional<at::Tensor>& bias,
                                         int64_t sh, int64_t sw, int64_t ph,
                                         int64_t pw) {
  auto out = conv2d_fwd_impl(x, w, bias, sh, sw, ph, pw, /*relu=*/false, true);
  if (out[1].numel()) {
    // partials -> [2, Cout], the fold bn_fwd_train does on the partials
    auto stats = at::empty({2, out[1].size(2)}, out[1].options());
    slab_fin_launch(out[1].data_ptr<float>(), stats.data_ptr<float>(),
                    (int)out[1].size(0), (int)(2 * out[1].size(2)),
                    cur_stream());
    out[1] = stats;
  }
  return out;
}

// the same with the statistics left as partials [m-tiles, 2, Cout] (empty when
// ineligible), for bn_fwd_train(precomp=...), which folds them in its finalize
std::vector<at::Tensor> conv2d_fwd_partials(
    const at::Tensor& x, const at::Tensor& w,
    const c10::optional<at::Tensor>& bias, int64_t sh, int64_t sw, int64_t ph,
    int64_t pw) {
  return conv2d_fwd_impl(x, w, bias, sh, sw, ph, pw, /*relu=*/false, true);
}

at::Tensor conv2d_dgrad(const at::Tensor& dy, const at::Tensor& w, int64_t H,
                        int64_t W, int64_t sh, int64_t sw, int64_t ph,
                        int64_t pw) {
  auto cs = conv_dgrad_shape("conv2d_dgrad", dy, w, H, W, sh, sw, ph, pw);
  int KH = cs.KH, KW = cs.KW, Cin = cs.Cin, Cout = cs.Cout;
  auto dx = at::empty({cs.N, H, W, Cin}, dy.options());
  if (conv2d_dgrad_wants_db(dt_of(dy), dy.data_ptr(), cs)) {
    // double-buffered path: weight as [Cin][(kh,kw,co)] k-contiguous rows
    auto w_t2d = at::empty({Cin, (int64_t)KH * KW * Cout}, w.options());
    transpose_w_dgrad_launch(dt_of(w), w.data_ptr(), w_t2d.data_ptr(), KH * KW,
                             Cin, Cout, cur_stream());
    conv2d_dgrad_launch(dt_of(dy), dy.data_ptr(), nullptr, w_t2d.data_ptr(),
                        dx.data_ptr(), zero_page(dy), cs, cur_stream());
    return dx;
  }
  // dgrad consumes the weight as B[(kh,kw,co)][ci]: transpose once per call
  auto w_t = at::empty({KH, KW, Cout, Cin}, w.options());
  transpose_w_launch(dt_of(w), w.data_ptr(), w_t.data_ptr(), KH, KW, Cin, Cout,
                     cur_stream());
  conv2d_dgrad_launch(dt_of(dy), dy.data_ptr(), w_t.data_ptr(), nullptr,
                      dx.data_ptr(), zero_page(dy), cs, cur_stream());
  return dx;
}

// which kernel conv2d_fwd / conv2d_fwd_stats and conv2d_dgrad launch for these
// arguments (tests and profile notes name the route with these)
std::string conv2d_fwd_route_name(const at::Tensor& x, const at::Tensor& w,
                                  int64_t sh, int64_t sw, int64_t ph,
                                  int64_t pw, bool stats) {
  auto cs = conv_fwd_shape("conv2d_fwd_route", x, w, sh, sw, ph, pw);
  return conv2d_fwd_route(dt_of(x), x.data_ptr(), cs, stats);
}

std::string conv2d_dgrad_route_name(const at::Tensor& dy,
                                    const at::Tensor& w, int64_t H, int64_t W,
                                    int64_t sh, int64_t sw, int64_t ph,
                                    int64_t pw) {
  auto cs = conv_dgrad_shape("conv2d_dgrad_route", dy, w, H, W, sh, sw, ph,
                             pw);
  return conv2d_dgrad_route(dt_of(dy), dy.data_ptr(), cs);
}

// kernel name and split-M count of conv2d_wgrad / conv2d_wgrad_bias for these
// arguments (the same with and without the bias row)
std::tuple<std::string, int64_t> conv2d_wgrad_route_name(
    const at::Tensor& x, const at::Tensor& dy, int64_t KH, int64_t KW,
    int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  auto cs = conv_wgrad_shape("conv2d_wgrad_route", x, dy, KH, KW, sh, sw, ph,
                             pw);
  return {conv2d_wgrad_route(dt_of(x), x.data_ptr(), dy.data_ptr(), cs),
          conv2d_wgrad_zsplits(dt_of(x), x.data_ptr(), dy.data_ptr(), cs)};
}

// returns [KH*KW*Cin (+1 with bias), Cout]: dw rows, then the bias-gradient row
static at::Tensor conv2d_wgrad_rows(const at::Tensor& x, const at::Tensor& dy,
                                    int64_t KH, int64_t KW, int64_t sh,
                                    int64_t sw, int64_t ph, int64_t pw,
                                    bool out_in_dt, bool bias) {
  auto cs = conv_wgrad_shape("conv2d_wgrad", x, dy, KH, KW, sh, sw, ph, pw);
  DT out_dt = out_in_dt ? dt_of(x) : DT::F32;
  const int64_t rows = KH * KW * cs.Cin + (bias ? 1 : 0);
  auto out = at::empty({rows, (int64_t)cs.Cout},
                       out_dt == DT::F32 ? x.options().dtype(at::kFloat)
                                         : x.options());
  int z = conv2d_wgrad_zsplits(dt_of(x), x.data_ptr(), dy.data_ptr(), cs);
  at::Tensor ws;
  float* wsp = nullptr;
  if (z > 1 || out_dt != DT::F32) {
    ws = at::empty({(int64_t)z * rows * cs.Cout},
                   x.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  conv2d_wgrad_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), out.data_ptr(),
                      out_dt, wsp, z, zero_page(x), cs, bias, cur_stream());
  return out;
}

at::Tensor conv2d_wgrad(const at::Tensor& x, const at::Tensor& dy, int64_t KH,
                        int64_t KW, int64_t sh, int64_t sw, int64_t ph,
                        int64_t pw, bool out_in_dt) {
  return conv2d_wgrad_rows(x, dy, KH, KW, sh, sw, ph, pw, out_in_dt, false)
      .view({KH, KW, x.size(3), dy.size(3)});
}

// weight and bias gradient from one kernel + one reduce: the bias gradient
// sum_m dy is one more output row of the wgrad GEMM (x == 1), so dw and db
// are views of the same tensor
std::vector<at::Tensor> conv2d_wgrad_bias(const at::Tensor& x,
                                          const at::Tensor& dy, int64_t KH,
                                          int64_t KW, int64_t sh, int64_t sw,
                                          int64_t ph, int64_t pw,
                                          bool out_in_dt) {
  auto out = conv2d_wgrad_rows(x, dy, KH, KW, sh, sw, ph, pw, out_in_dt, true);
  const int64_t kout = out.size(0) - 1;
  return {out.narrow(0, 0, kout).view({KH, KW, x.size(3), dy.size(3)}),
          out.select(0, kout)};
}

// A gradient destination handed to an into-variant: a contiguous GPU tensor
// of the given dtype and shape, on the operand's device.
static void check_grad_dst(const char* fn, const char* name,
                           const at::Tensor& t, const at::Tensor& like,
                           at::ScalarType st, at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), fn, ": ", name,
              " must be a GPU tensor on ", like.device());
  TORCH_CHECK(t.scalar_type() == st, fn, ": ", name, " must be ", st, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, fn, ": ", name, " must have shape ", shape,
              ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// splitk_reduce_can_split on plain integers (host arithmetic only; the
// addresses are byte addresses): whether a reduce of n elements can put
// [0, n0) at addr0 and [n0, n) at addr1 for fp32 (or bf16) output
bool splitk_can_split(int64_t n, int64_t n0, int64_t addr0, int64_t addr1,
                      bool bf16_out) {
  return splitk_reduce_can_split(n, n0, (const void*)(uintptr_t)addr0,
                                 (const void*)(uintptr_t)addr1,
                                 bf16_out ? DT::BF16 : DT::F32);
}

// conv2d_wgrad / conv2d_wgrad_bias with the split reduce writing straight
// into the parameters' gradient buffers: dw_out [KH, KW, Cin, Cout] and
// db_out [Cout] (optional), both of one dtype (x's, or fp32). accumulate adds
// the fp32 sum to what they hold and rounds once. Route, z and workspace are
// those of conv2d_wgrad_bias, so the bits are too.
void conv2d_wgrad_into(const at::Tensor& x, const at::Tensor& dy, int64_t KH,
                       int64_t KW, int64_t sh, int64_t sw, int64_t ph,
                       int64_t pw, at::Tensor dw_out,
                       const c10::optional<at::Tensor>& db_out,
                       bool accumulate) {
  const char* fn = "conv2d_wgrad_into";
  auto cs = conv_wgrad_shape(fn, x, dy, KH, KW, sh, sw, ph, pw);
  const auto st = dw_out.scalar_type();
  TORCH_CHECK(st == x.scalar_type() || st == at::kFloat, fn,
              ": dw_out must be ", x.scalar_type(), " or Float, got ", st);
  check_grad_dst(fn, "dw_out", dw_out, x, st,
                 {KH, KW, (int64_t)cs.Cin, (int64_t)cs.Cout});
  const bool bias = db_out.has_value();
  if (bias) check_grad_dst(fn, "db_out", *db_out, x, st, {(int64_t)cs.Cout});
  const DT out_dt = st == at::kFloat ? DT::F32 : dt_of(x);
  const int64_t kout = KH * KW * cs.Cin;
  const int64_t rows = kout + (bias ? 1 : 0);
  const int z = conv2d_wgrad_zsplits(dt_of(x), x.data_ptr(), dy.data_ptr(), cs);
  auto ws = at::empty({(int64_t)z * rows * cs.Cout},
                      x.options().dtype(at::kFloat));
  void* dbp = bias ? db_out->data_ptr() : nullptr;
  if (splitk_reduce_can_split(rows * cs.Cout, kout * cs.Cout,
                              dw_out.data_ptr(), bias ? dbp : dw_out.data_ptr(),
                              out_dt)) {
    WgradSink sink{dbp, accumulate};
    conv2d_wgrad_launch(dt_of(x), x.data_ptr(), dy.data_ptr(),
                        dw_out.data_ptr(), out_dt, ws.data_ptr<float>(), z,
                        zero_page(x), cs, bias, cur_stream(), &sink);
    return;
  }
  // the float4 reduce cannot split here (dw/db boundary or a destination off
  // a group of 4): reduce the old way into one fp32 tensor, then copy or add
  auto tmp = at::empty({rows, (int64_t)cs.Cout}, ws.options());
  WgradSink one{nullptr, false};
  conv2d_wgrad_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), tmp.data_ptr(),
                      DT::F32, ws.data_ptr<float>(), z, zero_page(x), cs, bias,
                      cur_stream(), &one);
  auto put = [&](at::Tensor dst, const at::Tensor& src) {
    dst.copy_(accumulate ? dst.to(at::kFloat).add_(src.view(dst.sizes()))
                         : src.view(dst.sizes()));
  };
  put(dw_out, tmp.narrow(0, 0, kout));
  if (bias) put(*db_out, tmp.select(0, kout));
}

// ---- batch norm ------------------------------------------------------------
std::vector<at::Tensor> bn_fwd_train(const at::Tensor& x,
                                     const at::Tensor& gamma,
                                     const at::Tensor& beta,
                                     const c10::optional<at::Tensor>& rmean,
                                     const c10::optional<at::Tensor>& rvar,
                                     double momentum, double eps, bool relu,
                                     double dropout_p, int64_t seed,
                                     const c10::optional<at::Tensor>& precomp,
                                     const c10::optional<at::Tensor>& ctr =
                                         c10::nullopt) {
  CHECK_IN(x);
  TORCH_CHECK(dropout_p == 0.0 || relu, "fused BN dropout requires relu");
  int C = x.size(-1);
  int64_t rows = x.numel() / C;
  auto mean = at::empty({C}, x.options().dtype(at::kFloat));
  auto invstd = at::empty({C}, x.options().dtype(at::kFloat));
  auto y = at::empty_like(x);
  float* rm = rmean.has_value() ? rmean->data_ptr<float>() : nullptr;
  float* rv = rvar.has_value() ? rvar->data_ptr<float>() : nullptr;
  if (precomp.has_value()) {
    // sums already produced by the conv epilogue: {2, C} (sum, sumsq), or
    // its slab partials {R, 2, C}, folded inside the finalize kernel
    TORCH_CHECK(precomp->is_cuda() && precomp->is_contiguous() &&
                    precomp->scalar_type() == at::kFloat,
                "bn_fwd_train: precomp must be a contiguous fp32 GPU tensor");
    const bool partials = precomp->dim() == 3;
    TORCH_CHECK(partials ? precomp->size(0) >= 1 && precomp->size(1) == 2 &&
                               precomp->size(2) == C
                         : precomp->numel() == 2 * C,
                "bad precomputed stats: ", precomp->sizes(), " for C = ", C);
    const float* ps = precomp->data_ptr<float>();
    if (partials)
      bn_finalize_fold_launch(ps, (int)precomp->size(0),
                              mean.data_ptr<float>(),
                              invstd.data_ptr<float>(), rm, rv,
                              (float)momentum, rows, C, (float)eps,
                              cur_stream());
    else
      bn_finalize_launch(ps, ps + C, mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), rm, rv, (float)momentum,
                         rows, C, (float)eps, cur_stream());
  } else {
    const int64_t wsn = bn_stats_ws_floats(dt_of(x), x.data_ptr(), rows, C);
    at::Tensor ws;
    float* wp = nullptr;
    if (wsn) {
      ws = at::empty({wsn}, x.options().dtype(at::kFloat));
      wp = ws.data_ptr<float>();
    }
    bn_stats_launch(dt_of(x), x.data_ptr(), mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), rm, rv, (float)momentum, wp,
                    rows, C, (float)eps, cur_stream());
  }
  if (dropout_p > 0.0)
    bn_apply_drop_launch(dt_of(x), x.data_ptr(), mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                         beta.data_ptr<float>(), y.data_ptr(), rows, C,
                         (float)dropout_p, (uint64_t)seed,
                         ctr.has_value() ? ctr->data_ptr<int64_t>() : nullptr,
                         cur_stream());
  else
    bn_apply_launch(dt_of(x), x.data_ptr(), mean.data_ptr<float>(),
                    invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                    beta.data_ptr<float>(), y.data_ptr(), rows, C, relu,
                    cur_stream());
  return {y, mean, invstd};
}

at::Tensor bn_fwd_infer(const at::Tensor& x, const at::Tensor& gamma,
                        const at::Tensor& beta, const at::Tensor& rmean,
                        const at::Tensor& rvar, double eps, bool relu) {
  CHECK_IN(x);
  int C = x.size(-1);
  int64_t rows = x.numel() / C;
  auto y = at::empty_like(x);
  bn_infer_launch(dt_of(x), x.data_ptr(), rmean.data_ptr<float>(),
                  rvar.data_ptr<float>(), gamma.data_ptr<float>(),
                  beta.data_ptr<float>(), y.data_ptr(), rows, C, (float)eps,
                  relu, cur_stream());
  return y;
}

std::vector<at::Tensor> bn_bwd(const at::Tensor& x, const at::Tensor& dy,
                               const at::Tensor& gamma, const at::Tensor& mean,
                               const at::Tensor& invstd,
                               const c10::optional<at::Tensor>& y_relu,
                               double dy_scale,
                               const c10::optional<at::Tensor>& resid =
                                   c10::nullopt,
                               const c10::optional<at::Tensor>& dgamma_out =
                                   c10::nullopt,
                               const c10::optional<at::Tensor>& dbeta_out =
                                   c10::nullopt,
                               bool accumulate = false) {
  CHECK_IN(x);
  CHECK_IN(dy);
  const void* resp = nullptr;
  if (resid.has_value()) {
    TORCH_CHECK(resid->is_contiguous() &&
                resid->scalar_type() == x.scalar_type() &&
                resid->numel() == x.numel(), "bn_bwd resid mismatch");
    resp = resid->data_ptr();
  }
  int C = x.size(-1);
  int64_t rows = x.numel() / C;
  const int64_t wsn = bn_bwd_ws_floats(dt_of(x), x.data_ptr(),
                                       dy.data_ptr(), rows, C);
  // slab path (vec) needs no zero-init; scalar fallback atomically
  // accumulates into zeroed sums
  auto sums = wsn ? at::empty({2, C}, x.options().dtype(at::kFloat))
                  : at::zeros({2, C}, x.options().dtype(at::kFloat));
  auto sum_dy = sums[0];
  auto sum_dy_xhat = sums[1];
  // gradient sinks: the slab finalize also writes (or adds) dgamma / dbeta
  // into these fp32 [C] buffers. Slab path only (bn_bwd_takes_sink): the
  // scalar-atomics fallback returns its sums and nothing else.
  float *dgp = nullptr, *dbp = nullptr;
  TORCH_CHECK(dgamma_out.has_value() == dbeta_out.has_value(),
              "bn_bwd: dgamma_out and dbeta_out go together");
  if (dgamma_out.has_value()) {
    TORCH_CHECK(wsn, "bn_bwd: no gradient sink on the scalar path "
                     "(ask bn_bwd_takes_sink first)");
    check_grad_dst("bn_bwd", "dgamma_out", *dgamma_out, x, at::kFloat, {C});
    check_grad_dst("bn_bwd", "dbeta_out", *dbeta_out, x, at::kFloat, {C});
    dgp = dgamma_out->data_ptr<float>();
    dbp = dbeta_out->data_ptr<float>();
  }
  at::Tensor ws;
  float* wp = nullptr;
  if (wsn) {
    ws = at::empty({wsn}, x.options().dtype(at::kFloat));
    wp = ws.data_ptr<float>();
  }
  auto dx = at::empty_like(x);
  const void* yr = y_relu.has_value() ? y_relu->data_ptr() : nullptr;
  bn_bwd_reduce_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), yr,
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       sum_dy.data_ptr<float>(), sum_dy_xhat.data_ptr<float>(),
                       wp, rows, C, (float)dy_scale, cur_stream(), dgp, dbp,
                       accumulate);
  bn_bwd_apply_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), yr,
                      mean.data_ptr<float>(), invstd.data_ptr<float>(),
                      gamma.data_ptr<float>(), sum_dy.data_ptr<float>(),
                      sum_dy_xhat.data_ptr<float>(), dx.data_ptr(), resp,
                      rows, C, (float)dy_scale, cur_stream());
  // dgamma = sum_dy_xhat, dbeta = sum_dy (fp32, matching fp32 gamma/beta)
  return {dx, sum_dy_xhat, sum_dy};
}

// whether bn_bwd of these operands runs the slab path, which alone can write
// dgamma_out / dbeta_out
bool bn_bwd_takes_sink(const at::Tensor& x, const at::Tensor& dy) {
  CHECK_IN(x);
  CHECK_IN(dy);
  const int C = x.size(-1);
  return bn_bwd_ws_floats(dt_of(x), x.data_ptr(), dy.data_ptr(),
                          x.numel() / C, C) != 0;
}

// ---- pooling ---------------------------------------------------------------
static PoolShape pool_shape(const at::Tensor& x, int KH, int KW, int SH, int SW,
                            int PH, int PW) {
  PoolShape ps;
  ps.N = x.size(0);
  ps.H = x.size(1);
  ps.W = x.size(2);
  ps.C = x.size(3);
  ps.KH = KH;
  ps.KW = KW;
  ps.SH = SH;
  ps.SW = SW;
  ps.PH = PH;
  ps.PW = PW;
  ps.OH = (ps.H + 2 * PH - KH) / SH + 1;
  ps.OW = (ps.W + 2 * PW - KW) / SW + 1;
  return ps;
}

std::vector<at::Tensor> maxpool_fwd(const at::Tensor& x, int64_t kh, int64_t kw,
                                    int64_t sh, int64_t sw, int64_t ph,
                                    int64_t pw) {
  CHECK_IN(x);
  auto ps = pool_shape(x, kh, kw, sh, sw, ph, pw);
  auto y = at::empty({ps.N, ps.OH, ps.OW, ps.C}, x.options());
  auto idx = at::empty({ps.N, ps.OH, ps.OW, ps.C}, x.options().dtype(at::kInt));
  maxpool_fwd_launch(dt_of(x), x.data_ptr(), y.data_ptr(), idx.data_ptr<int>(),
                     ps, cur_stream());
  return {y, idx};
}

at::Tensor maxpool_bwd(const at::Tensor& dy, const at::Tensor& idx, int64_t H,
                       int64_t W) {
  CHECK_IN(dy);
  PoolShape ps;
  ps.N = dy.size(0);
  ps.OH = dy.size(1);
  ps.OW = dy.size(2);
  ps.C = dy.size(3);
  ps.H = H;
  ps.W = W;
  auto dxf = at::zeros({ps.N, H, W, ps.C}, dy.options().dtype(at::kFloat));
  maxpool_bwd_launch(dt_of(dy), dy.data_ptr(), idx.data_ptr<int>(),
                     dxf.data_ptr<float>(), ps, cur_stream());
  if (dy.scalar_type() == at::kFloat) return dxf;
  auto dx = at::empty({ps.N, H, W, ps.C}, dy.options());
  cast_f32_launch(dt_of(dy), dxf.data_ptr<float>(), dx.data_ptr(), dx.numel(),
                  cur_stream());
  return dx;
}

at::Tensor avgpool_fwd(const at::Tensor& x, int64_t kh, int64_t kw, int64_t sh,
                       int64_t sw, int64_t ph, int64_t pw) {
  CHECK_IN(x);
  auto ps = pool_shape(x, kh, kw, sh, sw, ph, pw);
  auto y = at::empty({ps.N, ps.OH, ps.OW, ps.C}, x.options());
  avgpool_fwd_launch(dt_of(x), x.data_ptr(), y.data_ptr(), ps, cur_stream());
  return y;
}

at::Tensor avgpool_bwd(const at::Tensor& dy, int64_t H, int64_t W, int64_t kh,
                       int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                       int64_t pw) {
  CHECK_IN(dy);
  PoolShape ps;
  ps.N = dy.size(0);
  ps.OH = dy.size(1);
  ps.OW = dy.size(2);
  ps.C = dy.size(3);
  ps.H = H;
  ps.W = W;
  ps.KH = kh;
  ps.KW = kw;
  ps.SH = sh;
  ps.SW = sw;
  ps.PH = ph;
  ps.PW = pw;
  auto dx = at::empty({ps.N, H, W, ps.C}, dy.options());
  avgpool_bwd_launch(dt_of(dy), dy.data_ptr(), dx.data_ptr(), ps, cur_stream());
  return dx;
}

// ---- loss ------------------------------------------------------------------
std::vector<at::Tensor> ce_fwd(const at::Tensor& logits,
                               const at::Tensor& targets) {
  CHECK_IN(logits);
  CHECK_IN(targets);
  int64_t rows = logits.size(0);
  int cols = logits.size(1);
  auto loss = at::empty({rows}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({rows}, logits.options().dtype(at::kFloat));
  ce_fwd_launch(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(),
                loss.data_ptr<float>(), lse.data_ptr<float>(), rows, cols,
                cur_stream());
  return {loss, lse};
}

at::Tensor ce_bwd(const at::Tensor& logits, const at::Tensor& targets,
                  const at::Tensor& lse, const at::Tensor& dloss) {
  CHECK_IN(logits);
  auto dl = at::empty_like(logits);
  ce_bwd_launch(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(),
                lse.data_ptr<float>(), dloss.contiguous().data_ptr<float>(),
                dl.data_ptr(), logits.size(0), logits.size(1), cur_stream());
  return dl;
}

at::Tensor ptloss_fwd(const at::Tensor& pred, const at::Tensor& tgt,
                      int64_t kind, double delta) {
  CHECK_IN(pred);
  CHECK_IN(tgt);
  TORCH_CHECK(pred.sizes() == tgt.sizes(), "pred/target shape mismatch");
  auto out = at::zeros({}, pred.options().dtype(at::kFloat));
  ptloss_fwd_launch(dt_of(pred), pred.data_ptr(), tgt.data_ptr(),
                    out.data_ptr<float>(), pred.numel(), (int)kind,
                    (float)delta, cur_stream());
  return out;
}

at::Tensor ptloss_bwd(const at::Tensor& pred, const at::Tensor& tgt,
                      const at::Tensor& dloss, int64_t kind, double delta) {
  CHECK_IN(pred);
  auto dpred = at::empty_like(pred);
  ptloss_bwd_launch(dt_of(pred), pred.data_ptr(), tgt.data_ptr(),
                    dloss.contiguous().data_ptr<float>(), dpred.data_ptr(),
                    pred.numel(), (int)kind, (float)delta, cur_stream());
  return dpred;
}

// ---- group norm ------------------------------------------------------------
// x [N, ..., C] NHWC-contiguous; gamma/beta fp32 [C]
std::vector<at::Tensor> gn_fwd(const at::Tensor& x, const at::Tensor& gamma,
                               const at::Tensor& beta, int64_t groups,
                               double eps) {
  CHECK_IN(x);
  const int C = x.size(-1);
  const int64_t N = x.size(0);
  const int64_t HW = x.numel() / (N * C);
  TORCH_CHECK(C % groups == 0, "C % groups != 0");
  auto y = at::empty_like(x);
  auto mean = at::empty({N * groups}, x.options().dtype(at::kFloat));
  auto invstd = at::empty_like(mean);
  gn_fwd_launch(dt_of(x), x.data_ptr(), gamma.data_ptr<float>(),
                beta.data_ptr<float>(), y.data_ptr(), mean.data_ptr<float>(),
                invstd.data_ptr<float>(), N, HW, C, (int)groups, (float)eps,
                cur_stream());
  return {y, mean, invstd};
}

std::vector<at::Tensor> gn_bwd(const at::Tensor& x, const at::Tensor& dy,
                               const at::Tensor& mean, const at::Tensor& invstd,
                               const at::Tensor& gamma, int64_t groups) {
  CHECK_IN(x);
  CHECK_IN(dy);
  const int C = x.size(-1);
  const int64_t N = x.size(0);
  const int64_t HW = x.numel() / (N * C);
  auto dx = at::empty_like(x);
  auto s1 = at::empty({N * groups}, x.options().dtype(at::kFloat));
  auto s2 = at::empty_like(s1);
  auto dgamma = at::zeros({C}, x.options().dtype(at::kFloat));
  auto dbeta = at::zeros({C}, x.options().dtype(at::kFloat));
  gn_bwd_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), mean.data_ptr<float>(),
                invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                s1.data_ptr<float>(), s2.data_ptr<float>(), dx.data_ptr(),
                dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), N, HW, C,
                (int)groups, cur_stream());
  return {dx, dgamma, dbeta};
}

// ---- layer norm ------------------------------------------------------------
std::vector<at::Tensor> ln_fwd(const at::Tensor& x, const at::Tensor& gamma,
                               const at::Tensor& beta, double eps) {
  CHECK_IN(x);
  int cols = x.size(-1);
  int64_t rows = x.numel() / cols;
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto invstd = at::empty({rows}, x.options().dtype(at::kFloat));
  ln_fwd_launch(dt_of(x), x.data_ptr(), gamma.data_ptr<float>(),
                beta.data_ptr<float>(), y.data_ptr(), mean.data_ptr<float>(),
                invstd.data_ptr<float>(), rows, cols, (float)eps, cur_stream());
  return {y, mean, invstd};
}

std::vector<at::Tensor> ln_bwd(const at::Tensor& x, const at::Tensor& dy,
                               const at::Tensor& gamma, const at::Tensor& mean,
                               const at::Tensor& invstd,
                               const c10::optional<at::Tensor>& resid =
                                   c10::nullopt) {
  CHECK_IN(x);
  CHECK_IN(dy);
  const void* rp = nullptr;
  if (resid.has_value()) {
    TORCH_CHECK(resid->is_contiguous() &&
                resid->scalar_type() == x.scalar_type() &&
                resid->numel() == x.numel(), "ln_bwd resid mismatch");
    rp = resid->data_ptr();
  }
  int cols = x.size(-1);
  int64_t rows = x.numel() / cols;
  auto dx = at::empty_like(x);
  const int64_t wsn = ln_bwd_ws_floats(dt_of(x), x.data_ptr(), dy.data_ptr(),
                                       rows, cols);
  const bool vec = (dt_of(x) == DT::F32 ? cols % 4 == 0 : cols % 8 == 0) &&
                   ((uintptr_t)x.data_ptr() & 15) == 0 &&
                   ((uintptr_t)dy.data_ptr() & 15) == 0;
  // vec path single-writes (or slab-folds) the [2, cols] buffer; the
  // scalar fallback atomically accumulates into zeros
  auto sums = vec ? at::empty({2, cols}, x.options().dtype(at::kFloat))
                  : at::zeros({2, cols}, x.options().dtype(at::kFloat));
  at::Tensor ws;
  float* wp = nullptr;
  if (wsn) {
    ws = at::empty({wsn}, x.options().dtype(at::kFloat));
    wp = ws.data_ptr<float>();
  }
  ln_bwd_launch(dt_of(x), x.data_ptr(), dy.data_ptr(), gamma.data_ptr<float>(),
                mean.data_ptr<float>(), invstd.data_ptr<float>(), dx.data_ptr(),
                rp, sums.data_ptr<float>(), wp, rows, cols, cur_stream());
  return {dx, sums[0], sums[1]};
}

// ---- embedding -------------------------------------------------------------
at::Tensor embedding_fwd(const at::Tensor& ids, const at::Tensor& table) {
  CHECK_IN(ids);
  CHECK_IN(table);
  auto sizes = ids.sizes().vec();
  sizes.push_back(table.size(1));
  auto y = at::empty(sizes, table.options());
  embedding_fwd_launch(dt_of(table), ids.data_ptr<int64_t>(), table.data_ptr(),
                       y.data_ptr(), ids.numel(), table.size(1), cur_stream());
  return y;
}

at::Tensor embedding_bwd(const at::Tensor& ids, const at::Tensor& dy,
                         int64_t rows) {
  CHECK_IN(ids);
  CHECK_IN(dy);
  int dim = dy.size(-1);
  auto dt = at::zeros({rows, dim}, dy.options().dtype(at::kFloat));
  embedding_bwd_launch(dt_of(dy), ids.data_ptr<int64_t>(), dy.data_ptr(),
                       dt.data_ptr<float>(), ids.numel(), dim, cur_stream());
  return dt;
}

// ---- flash attention -------------------------------------------------------
// q/k/v/o/dout are [B,H,S,D] views that may be non-contiguous as long as
// d stays contiguous: BHSD-dense tensors, transposed views of BSHD
// buffers, or head-slices of one merged [B,S,3*H*D] QKV buffer. The
// kernels read rows through {row, head, batch} stride tuples, so no
// transpose/contiguous copies happen anywhere in the attention path.
static bool attn_view_ok(const at::Tensor& t, bool need_align) {
  if (t.stride(3) != 1) return false;
  if (!need_align) return true;  // scalar reads/writes: any row alignment
  // glds stages 16-B vectors: rows must stay 16-B aligned across s and h
  return t.stride(2) % 8 == 0 && t.stride(1) % 8 == 0 &&
         ((uintptr_t)t.data_ptr() & 15) == 0;
}

static std::array<int64_t, 3> attn_strides(const at::Tensor& t) {
  return {t.stride(2), t.stride(1), t.stride(0)};
}

// the kernels take one {B,H,S,D} and one stride tuple for q, k and v and
// trust every other tensor to match them: check all of it before a launch
static void attn_check_like(const char* fn, const char* name,
                            const at::Tensor& t, const at::Tensor& q,
                            at::IntArrayRef sizes, at::ScalarType dtype) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device(), fn, ": ", name,
              " must be on q's GPU (", q.device(), "), got ", t.device());
  TORCH_CHECK(t.scalar_type() == dtype, fn, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == sizes, fn, ": ", name, " must be ", sizes,
              ", got ", t.sizes());
}

static void attn_check_qkv(const char* fn, const at::Tensor& q,
                           const at::Tensor& k, const at::Tensor& v) {
  TORCH_CHECK(q.is_cuda(), fn, ": q must be on GPU");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, fn,
              ": flash attention is bf16, got q ", q.scalar_type());
  TORCH_CHECK(q.dim() == 4, fn, ": q must be [B,H,S,D]");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128, fn,
              ": head dim must be 64 or 128, got ", q.size(3));
  attn_check_like(fn, "k", k, q, q.sizes(), at::kBFloat16);
  attn_check_like(fn, "v", v, q, q.sizes(), at::kBFloat16);
}

std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 bool causal) {
  attn_check_qkv("attn_fwd", q, k, v);
  int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const bool strided_ok = attn_view_ok(q, true) && attn_view_ok(k, true) &&
                          attn_view_ok(v, true) &&
                          q.strides() == k.strides() &&
                          k.strides() == v.strides();
  if (!strided_ok) {
    q = q.contiguous(); k = k.contiguous(); v = v.contiguous();
  }
  // o lands BSHD-contiguous so the caller's transpose+reshape to
  // [B,S,H*D] is a free view
  auto o_buf = at::empty({B, S, (int64_t)H * D}, q.options());
  auto o = o_buf.view({B, S, H, D}).permute({0, 2, 1, 3});
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  float scale = 1.0f / std::sqrt((float)D);
  attn_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_buf.data_ptr(),
                  lse.data_ptr<float>(), zero_page(q), B, H, S, D,
                  attn_strides(q).data(), attn_strides(o).data(), causal,
                  scale, cur_stream());
  return {o, lse};
}

std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 const at::Tensor& o, at::Tensor dout,
                                 const at::Tensor& lse, bool causal,
                                 c10::optional<at::Tensor> dq_out,
                                 c10::optional<at::Tensor> dk_out,
                                 c10::optional<at::Tensor> dv_out) {
  attn_check_qkv("attn_bwd", q, k, v);
  attn_check_like("attn_bwd", "o", o, q, q.sizes(), at::kBFloat16);
  attn_check_like("attn_bwd", "dout", dout, q, q.sizes(), at::kBFloat16);
  attn_check_like("attn_bwd", "lse", lse, q, q.sizes().slice(0, 3),
                  at::kFloat);
  // the kernels index lse as [bh * S + row]
  TORCH_CHECK(lse.is_contiguous(), "attn_bwd: lse must be contiguous");
  int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const bool in_ok = attn_view_ok(q, true) && attn_view_ok(k, true) &&
                     attn_view_ok(v, true) && q.strides() == k.strides() &&
                     k.strides() == v.strides();
  if (!in_ok) { q = q.contiguous(); k = k.contiguous(); v = v.contiguous(); }
  if (!attn_view_ok(dout, true)) dout = dout.contiguous();
  TORCH_CHECK(attn_view_ok(o, false), "o must be d-contiguous");
  at::Tensor dq, dk, dv;
  if (dq_out.has_value()) {
    TORCH_CHECK(dk_out.has_value() && dv_out.has_value(),
                "provide all three grad views or none");
    // caller-provided grad views (e.g. three slices of one merged dQKV
    // buffer: the fused-QKV backward writes it in place, no cat/pad)
    dq = *dq_out; dk = *dk_out; dv = *dv_out;
    attn_check_like("attn_bwd", "dq_out", dq, q, q.sizes(), at::kBFloat16);
    attn_check_like("attn_bwd", "dk_out", dk, q, q.sizes(), at::kBFloat16);
    attn_check_like("attn_bwd", "dv_out", dv, q, q.sizes(), at::kBFloat16);
    TORCH_CHECK(dq.strides() == dk.strides() && dk.strides() == dv.strides()
                    && dq.stride(3) == 1,
                "grad views must share a d-contiguous stride tuple");
  } else {
    auto mk = [&]() {
      return at::empty({B, S, (int64_t)H * D}, q.options())
          .view({B, S, H, D}).permute({0, 2, 1, 3});
    };
    dq = mk(); dk = mk(); dv = mk();
  }
  auto dqw = at::zeros({B, H, S, D}, q.options().dtype(at::kFloat));
  auto di = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  float scale = 1.0f / std::sqrt((float)D);
  attn_bwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  dout.data_ptr(), lse.data_ptr<float>(), di.data_ptr<float>(),
                  dqw.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                  dv.data_ptr(), zero_page(q), B, H, S, D,
                  attn_strides(q).data(), attn_strides(o).data(),
                  attn_strides(dout).data(), attn_strides(dq).data(), causal,
                  scale, cur_stream());
  return {dq, dk, dv};
}

// ---- optimizers ------------------------------------------------------------
// clip: the CLIP_STATE-float vector clip_finalize wrote; lr_dev: one float
static const float* clip_ptr(const c10::optional<at::Tensor>& clip) {
  if (!clip.has_value()) return nullptr;
  TORCH_CHECK(clip->is_cuda() && clip->is_contiguous() &&
                  clip->scalar_type() == at::kFloat &&
                  clip->numel() >= CLIP_STATE,
              "clip must be a contiguous fp32 GPU vector of ", (int)CLIP_STATE);
  return clip->data_ptr<float>();
}
static const float* lr_ptr(const c10::optional<at::Tensor>& lr_dev) {
  if (!lr_dev.has_value()) return nullptr;
  TORCH_CHECK(lr_dev->is_cuda() && lr_dev->scalar_type() == at::kFloat &&
                  lr_dev->numel() >= 1,
              "lr_dev must be an fp32 GPU scalar");
  return lr_dev->data_ptr<float>();
}

void sgd_step(at::Tensor param, at::Tensor master, const at::Tensor& grad,
              const c10::optional<at::Tensor>& momentum_buf, double lr,
              double momentum, double weight_decay, bool nesterov,
              const c10::optional<at::Tensor>& clip = c10::nullopt,
              const c10::optional<at::Tensor>& lr_dev = c10::nullopt) {
  CHECK_IN(param);
  bool has_master = master.data_ptr() != param.data_ptr();
  float* mb = momentum_buf.has_value() ? momentum_buf->data_ptr<float>()
                                       : nullptr;
  sgd_step_launch(dt_of(param), grad.data_ptr(), dt_of(grad), param.data_ptr(),
                  master.data_ptr<float>(), mb, param.numel(), (float)lr,
                  (float)momentum, (float)weight_decay, nesterov, has_master,
                  clip_ptr(clip), lr_ptr(lr_dev), cur_stream());
}

// Sum of squares of the gradients a descriptor lists: one fp32 partial per
// chunk into part[base .. base + chunks.numel()). desc holds `stride` int64
// per tensor, grad pointer in slot gslot, numel in slot nslot.
void grad_sumsq_mt(const at::Tensor& desc, const at::Tensor& chunks,
                   int64_t stride, int64_t gslot, int64_t nslot, int64_t dt_g,
                   at::Tensor part, int64_t base) {
  CHECK_IN(desc);
  CHECK_IN(chunks);
  CHECK_IN(part);
  TORCH_CHECK(desc.scalar_type() == at::kLong &&
                  chunks.scalar_type() == at::kLong &&
                  part.scalar_type() == at::kFloat,
              "grad_sumsq_mt: desc/chunks int64, part fp32");
  TORCH_CHECK(stride > 0 && gslot >= 0 && gslot < stride && nslot >= 0 &&
                  nslot < stride && desc.numel() % stride == 0,
              "grad_sumsq_mt: bad descriptor layout");
  TORCH_CHECK(dt_g == 0 || dt_g == 1, "grad_sumsq_mt: fp32/bf16 grads only");
  TORCH_CHECK(base >= 0 && base + chunks.numel() <= part.numel(),
              "grad_sumsq_mt: partial buffer too small");
  grad_sumsq_mt_launch((DT)dt_g, desc.data_ptr<int64_t>(),
                       chunks.data_ptr<int64_t>(), (int)chunks.numel(),
                       (int)stride, (int)gslot, (int)nslot,
                       part.data_ptr<float>() + base, cur_stream());
}

// Fold part[0 .. npart) in a fixed order (or take the already reduced
// sumsq_in) and write {sumsq, norm, coef, skip} into state.
void clip_finalize(const at::Tensor& part, int64_t npart, double max_norm,
                   at::Tensor state,
                   const c10::optional<at::Tensor>& skipped = c10::nullopt,
                   const c10::optional<at::Tensor>& sumsq_in = c10::nullopt) {
  CHECK_IN(part);
  CHECK_IN(state);
  TORCH_CHECK(part.scalar_type() == at::kFloat && npart >= 0 &&
                  npart <= part.numel(),
              "clip_finalize: part fp32 with at least npart elements");
  TORCH_CHECK(state.scalar_type() == at::kFloat &&
                  state.numel() >= CLIP_STATE,
              "clip_finalize: state fp32 x ", (int)CLIP_STATE);
  int64_t* sk = nullptr;
  if (skipped.has_value()) {
    TORCH_CHECK(skipped->is_cuda() && skipped->scalar_type() == at::kLong &&
                    skipped->numel() >= 1,
                "clip_finalize: skipped must be an int64 GPU scalar");
    sk = skipped->data_ptr<int64_t>();
  }
  const float* sin = nullptr;
  if (sumsq_in.has_value()) {
    TORCH_CHECK(sumsq_in->is_cuda() && sumsq_in->scalar_type() == at::kFloat &&
                    sumsq_in->numel() >= 1,
                "clip_finalize: sumsq_in must be an fp32 GPU scalar");
    sin = sumsq_in->data_ptr<float>();
  }
  clip_finalize_launch(part.data_ptr<float>(), (int)npart, sin,
                       (float)max_norm, state.data_ptr<float>(), sk,
                       cur_stream());
}

void adam_step(at::Tensor param, at::Tensor master, const at::Tensor& grad,
               at::Tensor m, at::Tensor v, int64_t step, double lr,
               double beta1, double beta2, double eps, double weight_decay,
               bool adamw,
               const c10::optional<at::Tensor>& step_dev = c10::nullopt,
               const c10::optional<at::Tensor>& clip = c10::nullopt,
               const c10::optional<at::Tensor>& lr_dev = c10::nullopt) {
  CHECK_IN(param);
  bool has_master = master.data_ptr() != param.data_ptr();
  const int64_t* sd =
      step_dev.has_value() ? step_dev->data_ptr<int64_t>() : nullptr;
  adam_step_launch(dt_of(param), grad.data_ptr(), dt_of(grad), param.data_ptr(),
                   master.data_ptr<float>(), m.data_ptr<float>(),
                   v.data_ptr<float>(), param.numel(), (int)step, sd,
                   (float)lr, (float)beta1, (float)beta2, (float)eps,
                   (float)weight_decay, adamw, has_master, clip_ptr(clip),
                   lr_ptr(lr_dev), cur_stream());
}

void adam_step_mt(const at::Tensor& desc, const at::Tensor& chunks,
                  int64_t dt_p, int64_t dt_g, bool has_master, int64_t step,
                  double lr, double beta1, double beta2, double eps,
                  double weight_decay, bool adamw,
                  const c10::optional<at::Tensor>& step_dev = c10::nullopt,
                  const c10::optional<at::Tensor>& clip = c10::nullopt,
                  const c10::optional<at::Tensor>& lr_dev = c10::nullopt) {
  CHECK_IN(desc);
  CHECK_IN(chunks);
  const int64_t* sd =
      step_dev.has_value() ? step_dev->data_ptr<int64_t>() : nullptr;
  adam_mt_launch((DT)dt_p, (DT)dt_g, has_master,
                 desc.data_ptr<int64_t>(), chunks.data_ptr<int64_t>(),
                 (int)chunks.numel(), (int)step, sd, (float)lr, (float)beta1,
                 (float)beta2, (float)eps, (float)weight_decay, adamw,
                 clip_ptr(clip), lr_ptr(lr_dev), cur_stream());
}

// ---- batched MFMA gemm -----------------------------------------------------
// a: logical [batch, M, K]; b: logical [batch, K, N]. Either operand may
// be a transpose VIEW (unit stride in dim -2 instead of -1) — the layout
// is read off the strides, the tensor-level analog of
// cublasGemmStridedBatchedEx's opA/opB (reference src/math/cuda/gemm.cu:84).
at::Tensor bmm(const at::Tensor& a_in, const at::Tensor& b_in) {
  TORCH_CHECK(a_in.dim() == 3 && b_in.dim() == 3, "bmm expects 3-D tensors");
  TORCH_CHECK(a_in.is_cuda() && b_in.is_cuda(), "bmm expects GPU tensors");
  TORCH_CHECK(a_in.scalar_type() == b_in.scalar_type(), "bmm dtype mismatch");
  auto norm = [](const at::Tensor& t) {
    return (t.stride(2) == 1 || t.stride(1) == 1) ? t : t.contiguous();
  };
  at::Tensor a = norm(a_in), b = norm(b_in);
  const int64_t batch = a.size(0), M = a.size(1), K = a.size(2), N = b.size(2);
  TORCH_CHECK(b.size(0) == batch && b.size(1) == K, "bmm shape mismatch");
  TORCH_CHECK(batch >= 1, "bmm: empty operand (batch = 0)");
  CHECK_NONEMPTY("bmm", M, N, K);
  TORCH_CHECK(batch <= 65535, "bmm batch > 65535");
  bool ta, tb;
  int64_t lda, ldb;
  if (a.stride(2) == 1) { ta = false; lda = a.stride(1); }
  else { ta = true; lda = a.stride(2); }
  if (b.stride(2) == 1) { tb = false; ldb = b.stride(1); }
  else { tb = true; ldb = b.stride(2); }
  TORCH_CHECK(lda <= INT32_MAX && ldb <= INT32_MAX && M <= INT32_MAX &&
              N <= INT32_MAX && K <= INT32_MAX, "bmm dims exceed int32");
  auto c = at::empty({batch, M, N}, a.options());
  bmm_launch(dt_of(a), a.data_ptr(), b.data_ptr(), c.data_ptr(), zero_page(a),
             (int)batch, (int)M, (int)N, (int)K, (int)lda, (int)ldb, (int)N,
             a.stride(0), b.stride(0), M * N, ta, tb, cur_stream());
  return c;
}

// ---- scaled / causal softmax ----------------------------------------------
at::Tensor smax_fwd(const at::Tensor& x, int64_t mrows, int64_t qoff,
                    double scale, bool causal) {
  CHECK_IN(x);
  const int cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  auto y = at::empty_like(x);
  smax_fwd_launch(dt_of(x), x.data_ptr(), y.data_ptr(), rows, cols,
                  (int)mrows, (int)qoff, (float)scale, causal, cur_stream());
  return y;
}

at::Tensor smax_bwd(const at::Tensor& p, const at::Tensor& dy, double scale) {
  CHECK_IN(p);
  CHECK_IN(dy);
  const int cols = p.size(-1);
  const int64_t rows = p.numel() / cols;
  auto dx = at::empty_like(p);
  smax_bwd_launch(dt_of(p), p.data_ptr(), dy.data_ptr(), dx.data_ptr(), rows,
                  cols, (float)scale, cur_stream());
  return dx;
}

// ---- fused decode attention ------------------------------------------------
// q [BH, D] bf16; k/v [BH, cap, D] bf16 full cache buffers. Either pos
// (device int64, len = pos+1 — graph-capturable) or len gives the live KV
// length. pos holds one shared position, or B of them (BH % B == 0): row
// bh then uses pos[bh / (BH / B)].
at::Tensor attn_decode(const at::Tensor& q, const at::Tensor& k,
                       const at::Tensor& v,
                       const c10::optional<at::Tensor>& pos, int64_t len,
                       double scale) {
  CHECK_IN(q);
  CHECK_IN(k);
  CHECK_IN(v);
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "attn_decode is bf16-only");
  const int BH = q.size(0), D = q.size(1), cap = k.size(1);
  TORCH_CHECK(D == 64 || D == 128, "attn_decode supports D in {64,128}");
  TORCH_CHECK(k.size(0) == BH && k.size(2) == D && v.sizes() == k.sizes());
  // split KV so the grid approaches the CU count (decode is latency-
  // bound; 12 heads x 1 split measured 22us/call): static from (BH, cap)
  // for hipGraph capture
  int splits = std::max<int>(1, std::min<int>(16, 256 / BH));
  const int64_t* pos_ptr = nullptr;
  int pos_div = 0;  // 0: one shared position
  if (pos.has_value()) {
    TORCH_CHECK(pos->scalar_type() == at::kLong && pos->is_cuda());
    const int64_t nb = pos->numel();
    if (nb != 1) {
      TORCH_CHECK(nb >= 1 && pos->is_contiguous() && BH % nb == 0,
                  "attn_decode pos must hold 1 or B positions with BH % B "
                  "== 0, got ", nb, " for BH = ", BH);
      pos_div = (int)(BH / nb);
      // a batch brings B x heads rows, which the rule above would leave
      // unsplit (192 rows at B=16: one block walks a whole sequence, 31 us
      // per call); aim for ~4 blocks per CU instead. The shared-position
      // form keeps its split counts, and so its numerics.
      splits = std::max<int>(1, std::min<int>(16, 1024 / BH));
    }
    pos_ptr = pos->data_ptr<int64_t>();
  }
  auto po = at::empty({(int64_t)BH * splits, D},
                      q.options().dtype(at::kFloat));
  auto ml = at::empty({(int64_t)BH * splits, 2},
                      q.options().dtype(at::kFloat));
  auto out = at::empty_like(q);
  attn_decode_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                     po.data_ptr<float>(), ml.data_ptr<float>(),
                     out.data_ptr(), pos_ptr, pos_div, (int)len, BH, cap, D,
                     splits, (float)scale, cur_stream());
  return out;
}

// One launch writes sequence b's new K and V rows at pos[b], all heads.
// Caches [B,H,cap,D] contiguous; k_new / v_new [B,H,1,D] views with unit
// stride along D (the merged-QKV projection's slices); pos [B] int64 on
// device, trusted to be < cap.
void kv_append(at::Tensor& k_cache, at::Tensor& v_cache,
               const at::Tensor& k_new, const at::Tensor& v_new,
               const at::Tensor& pos) {
  CHECK_IN(k_cache);
  CHECK_IN(v_cache);
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
              v_cache.scalar_type() == k_cache.scalar_type(),
              "kv_append caches must be matching [B,H,cap,D]");
  const int64_t B = k_cache.size(0), H = k_cache.size(1),
                cap = k_cache.size(2), D = k_cache.size(3);
  for (const at::Tensor* t : {&k_new, &v_new}) {
    TORCH_CHECK(t->is_cuda() && t->dim() == 4 && t->size(0) == B &&
                t->size(1) == H && t->size(2) == 1 && t->size(3) == D &&
                (D == 1 || t->stride(3) == 1) &&
                t->scalar_type() == k_cache.scalar_type(),
                "kv_append new rows must be [B,H,1,D] views of the cache "
                "dtype with unit stride along D");
  }
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kLong &&
              pos.is_contiguous() && pos.numel() == B,
              "kv_append pos must be int64 [B] on device");
  kv_append_launch(dt_of(k_cache), k_cache.data_ptr(), v_cache.data_ptr(),
                   k_new.data_ptr(), v_new.data_ptr(),
                   pos.data_ptr<int64_t>(), (int)B, (int)H, (int)cap, (int)D,
                   k_new.stride(0), k_new.stride(1), v_new.stride(0),
                   v_new.stride(1), cur_stream());
}

// ---- extend attention / multi-row KV append --------------------------------
// Shared checks: caches are matching contiguous [B,H,cap,D] on the GPU;
// pos / n_new are contiguous device int64 [B]; 1 <= T <= cap.
static void ext_check_caches(const char* fn, const at::Tensor& kc,
                             const at::Tensor& vc) {
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() && kc.device() == vc.device(), fn,
              ": caches must be on one GPU");
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes() &&
              vc.scalar_type() == kc.scalar_type() && kc.is_contiguous() &&
              vc.is_contiguous(), fn,
              ": caches must be matching contiguous [B,H,cap,D]");
  TORCH_CHECK(kc.size(0) * kc.size(1) <= 65535, fn, ": B*H exceeds the grid");
}

static void ext_check_index(const char* fn, const char* name,
                            const at::Tensor& t, const at::Tensor& kc) {
  TORCH_CHECK(t.is_cuda() && t.device() == kc.device() &&
              t.scalar_type() == at::kLong && t.dim() == 1 &&
              t.numel() == kc.size(0) && t.is_contiguous(), fn, ": ", name,
              " must be contiguous int64 [B] on the caches' GPU");
}

static void ext_check_rows(const char* fn, const char* name,
                           const at::Tensor& t, const at::Tensor& kc) {
  TORCH_CHECK(t.is_cuda() && t.device() == kc.device(), fn, ": ", name,
              " must be on the caches' GPU");
  TORCH_CHECK(t.scalar_type() == kc.scalar_type(), fn, ": ", name,
              " must be ", kc.scalar_type(), ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.size(0) == kc.size(0) &&
              t.size(1) == kc.size(1) && t.size(3) == kc.size(3), fn, ": ",
              name, " must be [B,H,T,D] with the caches' B, H, D, got ",
              t.sizes());
  TORCH_CHECK(t.stride(3) == 1, fn, ": ", name,
              " must have unit stride along D");
  TORCH_CHECK(t.size(2) >= 1 && t.size(2) <= kc.size(2), fn,
              ": T must be in [1, cap], got ", t.size(2));
}

// q [B,H,T,D] bf16 view (unit d-stride, 16-byte aligned rows: the head
// slices of a merged [B,T,3*H*D] projection qualify) against the dense
// caches. Sequence b attends rows i < n_new[b] (all T when absent) at
// positions pos[b] + i over keys [0, pos[b] + i]; rows >= n_new[b] come
// back zero. o is [B,H,T,D] over [B,T,H,D] memory: o.transpose(1, 2) is
// contiguous. kv_splits == 0 runs k_attn_ext; kv_splits in [1, 16] (T <= 16
// only) runs the split-KV form with that many blocks per (b, h).
at::Tensor attn_extend(const at::Tensor& q, const at::Tensor& k_cache,
                       const at::Tensor& v_cache, const at::Tensor& pos,
                       const c10::optional<at::Tensor>& n_new, double scale,
                       int64_t kv_splits) {
  const char* fn = "attn_extend";
  TORCH_CHECK(kv_splits >= 0 && kv_splits <= 16, fn,
              ": kv_splits must be in [0, 16], got ", kv_splits);
  ext_check_caches(fn, k_cache, v_cache);
  TORCH_CHECK(k_cache.scalar_type() == at::kBFloat16, fn,
              ": bf16 only, got ", k_cache.scalar_type());
  const int64_t B = k_cache.size(0), H = k_cache.size(1),
                cap = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(D == 64 || D == 128, fn, ": head dim must be 64 or 128, got ",
              D);
  ext_check_rows(fn, "q", q, k_cache);
  TORCH_CHECK(attn_view_ok(q, true), fn,
              ": q rows must be 16-byte aligned across t, h and the base");
  ext_check_index(fn, "pos", pos, k_cache);
  if (n_new.has_value()) ext_check_index(fn, "n_new", *n_new, k_cache);
  const int64_t T = q.size(2);
  TORCH_CHECK(kv_splits == 0 || T <= 16, fn,
              ": kv_splits >= 1 wants T <= 16, got T = ", T);
  auto o_buf = at::empty({B, T, H * D}, q.options());
  auto o = o_buf.view({B, T, H, D}).permute({0, 2, 1, 3});
  if (kv_splits >= 1) {
    auto po = at::empty({B * H, kv_splits, 16, D},
                        q.options().dtype(at::kFloat));
    auto ml = at::empty({B * H, kv_splits, 16, 2},
                        q.options().dtype(at::kFloat));
    attn_ext_split_launch(
        q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        o_buf.data_ptr(), po.data_ptr<float>(), ml.data_ptr<float>(),
        pos.data_ptr<int64_t>(),
        n_new.has_value() ? n_new->data_ptr<int64_t>() : nullptr,
        zero_page(q), (int)B, (int)H, (int)T, (int)cap, (int)D,
        (int)kv_splits, attn_strides(q).data(), attn_strides(o).data(),
        (float)scale, cur_stream());
    return o;
  }
  attn_ext_launch(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                  o_buf.data_ptr(), pos.data_ptr<int64_t>(),
                  n_new.has_value() ? n_new->data_ptr<int64_t>() : nullptr,
                  zero_page(q), (int)B, (int)H, (int)T, (int)cap, (int)D,
                  attn_strides(q).data(), attn_strides(o).data(),
                  (float)scale, cur_stream());
  return o;
}

// k_new / v_new [B,H,T,D] views with unit d-stride (fp32 or bf16, the
// caches' dtype): rows i < n_new[b] go to cache slot pos[b] + i; slots
// >= cap and rows of a negative pos[b] are dropped.
void kv_append_n(at::Tensor& k_cache, at::Tensor& v_cache,
                 const at::Tensor& k_new, const at::Tensor& v_new,
                 const at::Tensor& pos,
                 const c10::optional<at::Tensor>& n_new) {
  const char* fn = "kv_append_n";
  ext_check_caches(fn, k_cache, v_cache);
  const auto dt = dt_of(k_cache);
  ext_check_rows(fn, "k_new", k_new, k_cache);
  ext_check_rows(fn, "v_new", v_new, k_cache);
  TORCH_CHECK(k_new.size(2) == v_new.size(2), fn,
              ": k_new and v_new disagree on T");
  ext_check_index(fn, "pos", pos, k_cache);
  if (n_new.has_value()) ext_check_index(fn, "n_new", *n_new, k_cache);
  const int64_t B = k_cache.size(0), H = k_cache.size(1),
                cap = k_cache.size(2), D = k_cache.size(3);
  const int64_t T = k_new.size(2);
  // 16-byte vectors need every row start aligned: bases, all three
  // strides and the row size
  const int64_t per = 16 / k_cache.element_size();
  auto vec_ok = [&](const at::Tensor& t) {
    return ((uintptr_t)t.data_ptr() & 15) == 0 && t.stride(0) % per == 0 &&
           t.stride(1) % per == 0 && t.stride(2) % per == 0;
  };
  const bool vec = D % per == 0 && vec_ok(k_new) && vec_ok(v_new) &&
                   vec_ok(k_cache) && vec_ok(v_cache);
  const std::array<int64_t, 3> ks = {k_new.stride(0), k_new.stride(1),
                                     k_new.stride(2)};
  const std::array<int64_t, 3> vs = {v_new.stride(0), v_new.stride(1),
                                     v_new.stride(2)};
  kv_append_n_launch(dt, k_cache.data_ptr(), v_cache.data_ptr(),
                     k_new.data_ptr(), v_new.data_ptr(),
                     pos.data_ptr<int64_t>(),
                     n_new.has_value() ? n_new->data_ptr<int64_t>() : nullptr,
                     (int)B, (int)H, (int)T, (int)cap, (int)D, ks.data(),
                     vs.data(), vec, cur_stream());
}

// ---- on-device sampling ----------------------------------------------------
// logits [R,V] bf16 -> ids [R] int64; step is a device int64 [1] (Philox
// counter, advanced in-graph by the caller); u [R] fp32 overrides the RNG.
at::Tensor sample_logits(const at::Tensor& logits, double temperature,
                         int64_t top_k, double top_p, int64_t seed,
                         const at::Tensor& step,
                         const c10::optional<at::Tensor>& u) {
  CHECK_IN(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.scalar_type() == at::kBFloat16,
              "sample_logits wants bf16 [R,V] logits");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (int64_t)1 << 31, "sample_logits: bad V ", V);
  TORCH_CHECK(temperature >= 0.0 && top_k >= 0 && top_p > 0.0 && top_p <= 1.0,
              "sample_logits wants temperature >= 0, top_k >= 0, top_p in "
              "(0, 1]");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kLong &&
              step.numel() == 1, "sample_logits step must be int64 [1]");
  const float* up = nullptr;
  if (u.has_value()) {
    TORCH_CHECK(u->is_cuda() && u->is_contiguous() &&
                u->scalar_type() == at::kFloat && u->numel() == R,
                "sample_logits u must be fp32 [R] on device");
    up = u->data_ptr<float>();
  }
  auto ids = at::empty({R}, logits.options().dtype(at::kLong));
  if (R > 0)
    sample_logits_launch(logits.data_ptr(), ids.data_ptr<int64_t>(), (int)R,
                         (int)V, (float)temperature,
                         (int)std::min<int64_t>(top_k, V), (float)top_p,
                         (uint64_t)seed, step.data_ptr<int64_t>(), up,
                         cur_stream());
  return ids;
}

namespace imgcodec {
at::Tensor decode_image(const py::bytes& data);  // imagecodec.cpp (host-only)
}

}  // namespace tnn

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("act_fwd", &tnn::act_fwd);
  m.def("act_bwd", &tnn::act_bwd);
  m.def("relu_bwd_mask", &tnn::relu_bwd_mask);
  m.def("add_act_fwd", &tnn::add_act_fwd);
  m.def("add_act_bwd", &tnn::add_act_bwd);
  m.def("dropout_fwd", &tnn::dropout_fwd, py::arg("x"), py::arg("p"),
        py::arg("seed"), py::arg("ctr") = c10::nullopt);
  m.def("dropout_bwd", &tnn::dropout_bwd);
  m.def("colsum", &tnn::colsum);
  m.def("gemm", &tnn::gemm, py::arg("a"), py::arg("b"), py::arg("bias"),
        py::arg("act_kind"), py::arg("residual") = c10::nullopt,
        py::arg("ln_gamma") = c10::nullopt, py::arg("ln_beta") = c10::nullopt,
        py::arg("ln_eps") = 1e-5);
  m.def("gemm_skinny", &tnn::gemm_skinny, py::arg("a"), py::arg("b"),
        py::arg("bias"), py::arg("act_kind"),
        py::arg("residual") = c10::nullopt, py::arg("ln_gamma") = c10::nullopt,
        py::arg("ln_beta") = c10::nullopt, py::arg("ln_eps") = 1e-5);
  m.def("skinny_enabled", &tnn::skinny_enabled);
  m.def("gemm_nt", &tnn::gemm_nt);
  m.def("gemm_tn", &tnn::gemm_tn);
  m.def("mfma_selftest", &tnn::mfma_selftest);
  m.def("mfma_selftest_f32", &tnn::mfma_selftest_f32);
  m.def("conv2d_fwd", &tnn::conv2d_fwd);
  m.def("conv2d_fwd_stats", &tnn::conv2d_fwd_stats);
  m.def("conv2d_fwd_partials", &tnn::conv2d_fwd_partials);
  m.def("conv2d_dgrad", &tnn::conv2d_dgrad);
  m.def("conv2d_fwd_route", &tnn::conv2d_fwd_route_name);
  m.def("conv2d_dgrad_route", &tnn::conv2d_dgrad_route_name);
  m.def("conv2d_wgrad_route", &tnn::conv2d_wgrad_route_name);
  m.def("conv2d_wgrad", &tnn::conv2d_wgrad);
  m.def("conv2d_wgrad_bias", &tnn::conv2d_wgrad_bias);
  m.def("conv2d_wgrad_into", &tnn::conv2d_wgrad_into, py::arg("x"),
        py::arg("dy"), py::arg("KH"), py::arg("KW"), py::arg("sh"),
        py::arg("sw"), py::arg("ph"), py::arg("pw"), py::arg("dw_out"),
        py::arg("db_out") = py::none(), py::arg("accumulate") = false);
  m.def("bn_bwd_takes_sink", &tnn::bn_bwd_takes_sink);
  m.def("splitk_can_split", &tnn::splitk_can_split);
  m.def("bn_fwd_train", &tnn::bn_fwd_train, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("rmean"), py::arg("rvar"),
        py::arg("momentum"), py::arg("eps"), py::arg("relu"),
        py::arg("dropout_p"), py::arg("seed"), py::arg("precomp"),
        py::arg("ctr") = c10::nullopt);
  m.def("bn_fwd_infer", &tnn::bn_fwd_infer);
  m.def("bn_bwd", &tnn::bn_bwd, py::arg("x"), py::arg("dy"),
        py::arg("gamma"), py::arg("mean"), py::arg("invstd"),
        py::arg("y_relu"), py::arg("dy_scale"),
        py::arg("resid") = py::none(), py::arg("dgamma_out") = py::none(),
        py::arg("dbeta_out") = py::none(), py::arg("accumulate") = false);
  m.def("maxpool_fwd", &tnn::maxpool_fwd);
  m.def("maxpool_bwd", &tnn::maxpool_bwd);
  m.def("avgpool_fwd", &tnn::avgpool_fwd);
  m.def("avgpool_bwd", &tnn::avgpool_bwd);
  m.def("ce_fwd", &tnn::ce_fwd);
  m.def("ce_bwd", &tnn::ce_bwd);
  m.def("ptloss_fwd", &tnn::ptloss_fwd);
  m.def("ptloss_bwd", &tnn::ptloss_bwd);
  m.def("gn_fwd", &tnn::gn_fwd);
  m.def("gn_bwd", &tnn::gn_bwd);
  m.def("ln_fwd", &tnn::ln_fwd);
  m.def("ln_bwd", &tnn::ln_bwd, py::arg("x"), py::arg("dy"),
        py::arg("gamma"), py::arg("mean"), py::arg("invstd"),
        py::arg("resid") = py::none());
  m.def("embedding_fwd", &tnn::embedding_fwd);
  m.def("embedding_bwd", &tnn::embedding_bwd);
  m.def("attn_fwd", &tnn::attn_fwd);
  m.def("attn_bwd", &tnn::attn_bwd, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("o"), py::arg("dout"), py::arg("lse"),
        py::arg("causal"), py::arg("dq_out") = py::none(),
        py::arg("dk_out") = py::none(), py::arg("dv_out") = py::none());
  m.def("bmm", &tnn::bmm);
  m.def("smax_fwd", &tnn::smax_fwd);
  m.def("smax_bwd", &tnn::smax_bwd);
  m.def("attn_decode", &tnn::attn_decode);
  m.def("kv_append", &tnn::kv_append);
  m.def("attn_extend", &tnn::attn_extend, py::arg("q"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("pos"), py::arg("n_new"),
        py::arg("scale"), py::arg("kv_splits") = 0);
  m.def("attn_extend_splits", &tnn::attn_ext_splits, py::arg("BH"),
        py::arg("cap"), py::arg("T"));
  m.def("kv_append_n", &tnn::kv_append_n);
  m.def("sample_logits", &tnn::sample_logits, py::arg("logits"),
        py::arg("temperature"), py::arg("top_k"), py::arg("top_p"),
        py::arg("seed"), py::arg("step"), py::arg("u") = c10::nullopt);
  m.def("sgd_step", &tnn::sgd_step, py::arg("param"), py::arg("master"),
        py::arg("grad"), py::arg("momentum_buf"), py::arg("lr"),
        py::arg("momentum"), py::arg("weight_decay"), py::arg("nesterov"),
        py::arg("clip") = c10::nullopt, py::arg("lr_dev") = c10::nullopt);
  m.def("adam_step", &tnn::adam_step, py::arg("param"), py::arg("master"),
        py::arg("grad"), py::arg("m"), py::arg("v"), py::arg("step"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("adamw"),
        py::arg("step_dev") = c10::nullopt, py::arg("clip") = c10::nullopt,
        py::arg("lr_dev") = c10::nullopt);
  m.def("adam_step_mt", &tnn::adam_step_mt, py::arg("desc"),
        py::arg("chunks"), py::arg("dt_p"), py::arg("dt_g"),
        py::arg("has_master"), py::arg("step"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("adamw"),
        py::arg("step_dev") = c10::nullopt, py::arg("clip") = c10::nullopt,
        py::arg("lr_dev") = c10::nullopt);
  m.def("grad_sumsq_mt", &tnn::grad_sumsq_mt, py::arg("desc"),
        py::arg("chunks"), py::arg("stride"), py::arg("gslot"),
        py::arg("nslot"), py::arg("dt_g"), py::arg("part"), py::arg("base"));
  m.def("clip_finalize", &tnn::clip_finalize, py::arg("part"),
        py::arg("npart"), py::arg("max_norm"), py::arg("state"),
        py::arg("skipped") = c10::nullopt, py::arg("sumsq_in") = c10::nullopt);
  m.def("decode_image", &tnn::imgcodec::decode_image);
}
