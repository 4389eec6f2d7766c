// Host-side launcher declarations shared by the kernel translation units and
// the PyTorch operator bindings (bindings.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "tune.h"  // tuning switches (in-process A/B experiments, the autotuner's overrides): named slots

typedef __bf16 bf16;

namespace dcp {

constexpr int kMaxTaps = 64;

struct TapList {
  int n;
  int dy[kMaxTaps], dx[kMaxTaps], widx[kMaxTaps];
};

// Backward of a training-mode BN + ReLU/identity (+ residual add) fused into the epilogue of
// the stride-1 dgrad that produces the gradient g of the BN layer's OUTPUT:
//   dst = g' = g * act'(y*scale + shift [+ res])   (the activation-masked gradient)
//   part[tile][0][c] = sum g',  part[tile][1][c] = sum g' * (y - mean) * invstd  (per 128-row tile)
// so the separate BN backward reduction pass (re-reading g and y) disappears.
struct BnBwdEpi {
  const bf16* y;        // BN input [M][C]; nullptr (with mask, act 1): not read, the xhat partials are zeros
  const bf16* res;      // residual added before the activation, or nullptr
  const float* scale;   // gamma * invstd
  const float* shift;   // beta - mean * scale
  const float* mean;
  const float* invstd;
  float* part;          // [ceil(M/128)][2][C]
  int act;              // 0 none, 1 ReLU (gradient stored masked), 2 leaky ReLU (stored RAW, summed masked)
  const uint8_t* mask;  // act'(z) > 0 as bits [M][C/8] (bn_act's mask output), or nullptr: recompute z
  float slope;          // leaky slope (act 2)
  // addsrc on the stride-2 subgrid only: [N][add_hc][add_wc][C] holds the gradient of the even
  // (y, x) pixels, zero elsewhere -- a projection block's 1x1 / stride-2 downsample dgrad, deposited
  // compact instead of as a mostly-zero full-size tensor (ops/functional.py StridedGrad)
  int add_s2;
  int add_hc, add_wc;
};

// Eval-mode BN folded into the forward conv's store epilogue (running statistics: model.eval(),
// NESTED's frozen BN): dst = act(acc_bf16 * scale + shift [+ addsrc]) per output channel, so the
// conv output is never written un-normalised and no separate BN-apply pass runs.
struct AffineEpi {
  const float* scale;  // gamma * invstd(running var)
  const float* shift;  // beta - running_mean * scale
  int act;             // 0 none, 1 ReLU, 2 leaky ReLU
  float slope;
};

// stream-ordered device workspace for kernels that need scratch (stream-K partials): bindings.cpp
// registers PyTorch's caching allocator (raw_alloc_with_stream / raw_delete)
using WorkspaceAlloc = void* (*)(size_t bytes, hipStream_t stream);
using WorkspaceFree = void (*)(void* ptr);
void set_workspace_allocator(WorkspaceAlloc alloc, WorkspaceFree free_fn);
// One implicit-GEMM ("tap GEMM") launch, forward or data gradient:
//   dst[n][oy + y*ds][ox + x*ds][co] = epilogue(sum over taps t, channels c of
//                                      src[n][y*ss + dy_t][x*ss + dx_t][c] * wt[co][widx_t][c])
// for the Hy x Wy output pixels (y, x) of each image; source pixels out of range read `zero`.
struct TapGemmProblem {
  // source [N][Hs][Ws][Cs]
  const bf16* src = nullptr;
  int N = 0, Hs = 0, Ws = 0, Cs = 0;
  // weight [Co][T][Cs] (with a second source: [Co][T*Cs + Cs2])
  const bf16* wt = nullptr;
  int Co = 0, T = 0;
  // destination [N][Hd][Wd][Co] and the output grid Hy x Wy computed by this launch: source stride ss,
  // destination stride ds and offset (oy, ox) -- a stride-2 data gradient writes one parity class per launch
  bf16* dst = nullptr;
  int Hd = 0, Wd = 0, Hy = 0, Wy = 0, ss = 1, ds = 1, oy = 0, ox = 0;
  const TapList* taps = nullptr;  // (read during the launch call only)
  // epilogue: BN statistics slabs [ceil(M/128)][2][Co] of the output; bias (fp32, its first nbias columns;
  // 0 = all Co) and relu (1 ReLU, 2 sigmoid: the linear layers); an add source shaped like dst; the fused
  // BN backward (BnBwdEpi) or the folded eval-mode BN (AffineEpi)
  float* stats = nullptr;
  const float* bias = nullptr;
  int nbias = 0, relu = 0;
  const bf16* addsrc = nullptr;
  const BnBwdEpi* bnb = nullptr;
  const AffineEpi* aff = nullptr;
  // prologue: BN + ReLU on the input of a 1x1 stride-1 forward, K5 -- the input is the BN's input x and
  // the conv sees bf16(relu(x * pscale[c] + pshift[c]))
  const float *pscale = nullptr, *pshift = nullptr;
  // second source: a second A operand concatenated along K -- a 1x1 source [pixels][Cs2] on src's pixel
  // grid, Cs2 % 64 == 0, against columns T*Cs .. of the weight; bias2, fp32 [Co], is added in fp32 before
  // the output's bf16 rounding.  Plain FAST store GEMMs only; never split-K.
  const bf16* src2 = nullptr;
  int Cs2 = 0;
  const float* bias2 = nullptr;
  const bf16* zero = nullptr;  // >= 256 zero bytes: the source of every out-of-bounds lane
};
void launch_tap_gemm(const TapGemmProblem& p, hipStream_t stream);
// number of problems the tap-GEMM autotuner (g_tune[kAutotune] = 1) has measured in this process
int tap_gemm_tuned_count();
// the tuner's per-problem choices as "tg\tkey\tchoice" lines, and back: the "tg" lines of `text`
// (returns entries accepted)
std::string tap_gemm_tune_export();
int tap_gemm_tune_import(const std::string& text);
// backward of act(c * scale + shift [+ r]) from its output y: g = dy * act'(y) and dc = g * scale
// (g only when want_g: the residual's gradient)
void launch_act_scale_bwd(const bf16* dy, const bf16* y, const float* scale, int64_t M, int C, int act, float slope,
                          bf16* dc, bf16* g, hipStream_t s);
void launch_partial_sum(const float* part, int P, int K, float* out, hipStream_t s);
void launch_partial_sum_bf16(const float* part, int P, int K, bf16* out, hipStream_t s);
// Weight gradient dw[co][t][c] = sum over output pixels of dy[n][y][x][co] * src[n][y*ss + dy_t][x*ss + dx_t][c]
struct WgradProblem {
  // output gradient [N][Ho][Wo][Co]
  const bf16* dy = nullptr;
  int N = 0, Ho = 0, Wo = 0, Co = 0;
  // conv input [N][Hs][Ws][Cs], source stride ss
  const bf16* src = nullptr;
  int Hs = 0, Ws = 0, Cs = 0, ss = 1;
  const TapList* taps = nullptr;  // (read during the call only)
  // BN + ReLU prologue on the input (as TapGemmProblem's): 1x1 stride-1, or the direct 3x3 kernel
  const float *pscale = nullptr, *pshift = nullptr;
  const bf16* zero = nullptr;
};
// splits (partials) of launch_wgrad for this problem: the direct 3x3 kernel's where it applies
int wgrad_plan_splits(const WgradProblem& p, int num_cu);
// floats of a split-K partial buffer for launch_split_reduce: `splits` rows of `row` floats and, behind
// them, the ceil(splits / 64) chunk sums of its two-level reduction
inline size_t split_part_elems(int splits, size_t row) { return (size_t)(splits + (splits + 63) / 64) * row; }
// wgrad3x3.hip: direct 3x3 / stride-1 / pad-1 weight gradient (0 = not applicable)
int wgrad3x3_splits(int N, int H, int W, int C, int Co, int num_cu);
void launch_wgrad3x3(const bf16* dy, const bf16* x, int N, int H, int W, int C, int Co, float* part, int splits,
                     const bf16* zero, hipStream_t stream, const float* pscale = nullptr,
                     const float* pshift = nullptr);
void launch_split_reduce(const float* part, int splits, int n, float* out, hipStream_t stream);
// partial-slab split-K weight gradient: dw [Co][T*Cs] is fully written when part != nullptr (part:
// split_part_elems(wgrad_plan_splits(p, num_cu), Co * T*Cs) floats); part == nullptr -> fp32 atomics into
// a zeroed dw
void launch_wgrad(const WgradProblem& p, float* dw, float* part, int num_cu, hipStream_t stream);
// frag: gconv_frag_elems(...) bf16 workspace (MFMA path; may be null -> direct kernels)
// stats (optional, [gconv_fwd_stat_blocks(M)][3][Co]): BN partials of y from the MFMA kernel's epilogue;
// returns whether they were written (false: the direct fallback kernel ran)
bool launch_grouped_conv_fwd(const bf16* x, const bf16* w, bf16* y, bf16* frag, int N, int H, int W, int C, int Ho,
                             int Wo, int Co, int G, int KH, int KW, int stride, int pad, hipStream_t s,
                             float* stats = nullptr);
int gconv_fwd_stat_blocks(int M);
void launch_grouped_conv_dgrad(const bf16* dy, const bf16* w, bf16* dx, bf16* frag, int N, int H, int W, int C,
                               int Ho, int Wo, int Co, int G, int KH, int KW, int stride, int pad, hipStream_t s);
// dw is fully written; part = workspace of gconv_mfma_wgrad_splits(...) x Co*KH*KW*(C/G) floats
void launch_grouped_conv_wgrad(const bf16* dy, const bf16* x, float* dw, float* part, int splits, const bf16* zero,
                               int N, int H, int W, int C, int Ho, int Wo, int Co, int G, int KH, int KW, int stride,
                               int pad, hipStream_t s);
// MFMA super-group kernels (gconv.hip); return false for shapes they do not cover
int gconv_frag_elems(int C, int G, int KH, int KW);
bool launch_gconv_mfma_fwd(const bf16* x, const bf16* w, bf16* y, bf16* frag, int N, int H, int W, int C, int Ho,
                           int Wo, int Co, int G, int KH, int KW, int stride, int pad, hipStream_t s,
                           float* stats = nullptr);
// fused ReLU-BN backward reduction for the grouped dgrad (z: BN input; part: [gconv_fwd_stat_blocks(M)][2][C])
struct GconvBnBwd {
  const bf16* z;
  const float *scale, *shift, *mean, *invstd;
  float* part;
};
bool launch_gconv_mfma_dgrad(const bf16* dy, const bf16* w, bf16* dx, bf16* frag, int N, int H, int W, int C, int Ho,
                             int Wo, int Co, int G, int KH, int KW, int stride, int pad, hipStream_t s,
                             const GconvBnBwd* bn = nullptr);
int gconv_mfma_wgrad_splits(int N, int Ho, int Wo, int C, int G);
int gconv_fallback_wgrad_splits(int M, int nw);  // part rows the direct fallback needs
bool launch_gconv_mfma_wgrad(const bf16* dy, const bf16* x, float* dw, float* part, int splits, const bf16* zero,
                             int N, int H, int W, int C, int Ho, int Wo, int Co, int G, int KH, int KW, int stride,
                             int pad, hipStream_t s);

int bn_stats_partials(int M, int C, bool from_slabs);
void launch_bn_stats(const bf16* x, const float* slabs, int M, int C, float* part, float* out, hipStream_t s);
// iabn_eps >= 0 (the finalize launchers): InplaceABN's |gamma| + iabn_eps as the weight, 1 / it into rgamma
void launch_bn_stats_finalize(const bf16* x, const float* slabs, int M, int C, float* part, float eps,
                              const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                              float* shift, float* rm, float* rv, float momentum, hipStream_t s, float iabn_eps = -1.f,
                              float* rgamma = nullptr);
// BN statistics from ready first-level partials [P][3][C] (e.g. the stem kernel's)
// two-level merge of many partials: chunks of 128 rows (0 = merge directly), and the first level
int bn_partial_chunks(int P);
void launch_bn_partial_chunk(const float* part, int P, int C, float* tmp, hipStream_t s);
void launch_bn_merge(const float* part, int P, int C, float* out, hipStream_t s);
void launch_bn_merge_finalize(const float* part, int P, int C, float eps, const float* gamma, const float* beta,
                              float* mean, float* invstd, float* scale, float* shift, float* rm, float* rv,
                              float momentum, hipStream_t s, float iabn_eps = -1.f, float* rgamma = nullptr);
// stem.hip: the space-to-depth stem conv [N][H][W][16] x [64][4][4][16] -> [N][H][W][64]
bool stem_fwd_supported(int H, int W, int C, int Co, int KH, int KW);
int stem_fwd_blocks(int N, int H);
void launch_stem_fwd(const bf16* x, const bf16* w, bf16* y, float* part, const bf16* zero, int N, int H, int W,
                     hipStream_t s);
// fused stem backward (BN + ReLU + 3x3/2 max pool + weight gradient): part [blocks][part_floats];
// reduce it over blocks (launch_split_reduce) -> tot, then sums [2][64] and dw [64][256]
bool stem_bwd_supported(int H, int W, int C, int Ho, int Wo);
int stem_bwd_blocks(int N, int H, int num_cu);
int stem_bwd_part_floats();
void launch_stem_bwd(const bf16* z, const bf16* x16, const bf16* dy, const uint8_t* idx, const float* scale,
                     const float* shift, const float* mean, int act, int N, int H, int W, int nblocks, float* part,
                     hipStream_t s);
void launch_stem_bwd_sums(const float* tot, const float* invstd, float* sums, hipStream_t s);
void launch_stem_bwd_dw(const float* tot, const float* sums, const float* scale, const float* invstd, float inv_count,
                        float* dw, hipStream_t s);
int colsum_partials(int M);
void launch_colsum(const bf16* x, int M, int C, float* part, float* out, hipStream_t s);
// bn_lin.hip: backward of a training-mode BN behind a 1x1 stride-1 conv (width m -> C channels) as a linear
// map of the conv's operands.  prep: coef [3][C] fp32 scratch, wcat [m][C + m] bf16 (the weight of the
// K-concatenated dgrad GEMM over [g | a2]) and its fp32 bias [m]; dw: the weight-gradient fix-up from
// G = g^T a2 [C][m] and A2 = a2^T a2 [m][m].  w3: [C][m] bf16 (forward layout), wt: [m][C] (transposed).
// colsum: column sums of a2 [M][m] (part: [bn_lin_colsum_partials][m] scratch); qpart: [bn_lin_q_slices][m][m].
bool bn_lin_supported(int m, int C);
int bn_lin_colsum_partials(int M, int m);
int bn_lin_q_slices(int m, int C);
void launch_bn_lin_colsum(const bf16* a2, int M, int m, float* part, float* out, hipStream_t s);
void launch_bn_lin_prep(const bf16* w3, const bf16* wt, const float* scale, const float* invstd, const float* sums,
                        const float* colsum, float inv_count, int m, int C, float* coef, float* qpart, bf16* wcat,
                        float* bias, hipStream_t s);
void launch_bn_lin_dw(const float* G, const float* A2, const bf16* w3, const float* coef, const float* colsum,
                      float inv_count, int m, int C, float* dw, hipStream_t s);
// s2: sums[1][c] = invstd[c] sum_k w3[c][k] (G[c][k] - sums[0][c] colsum[k] / n) (sum g xhat without the BN input)
void launch_bn_lin_s2(const float* G, const bf16* w3, const float* colsum, const float* invstd, float inv_count,
                      int m, int C, float* sums, hipStream_t s);
void launch_bn_finalize(const float* st, int W, int C, float eps, const float* gamma, const float* beta, float* mean,
                        float* invstd, float* scale, float* shift, float* rm, float* rv, float momentum,
                        hipStream_t s, float iabn_eps = -1.f, float* rgamma = nullptr);
void launch_bn_eval_coeff(int C, float eps, const float* gamma, const float* beta, const float* rm, const float* rv,
                          float* mean, float* invstd, float* scale, float* shift, hipStream_t s);
void launch_bn_act_fwd(const bf16* x, const bf16* res, const float* scale, const float* shift, bf16* y, size_t numel,
                       int C, int act, float slope, hipStream_t s, uint8_t* mask = nullptr,
                       const float* rscale = nullptr, const float* rshift = nullptr);
void launch_bn2_bwd_elemt(const bf16* dy, const bf16* x, const bf16* r, const float* scale, const float* mean,
                          const float* invstd, const float* sums, const float* rscale, const float* rmean,
                          const float* rinvstd, const float* rsums, float inv_count, size_t numel, int C, bf16* dx,
                          bf16* dr, hipStream_t s);
int bn_bwd_reduce_blocks(int M, int C);
void launch_bn_bwd_reduce(const bf16* dy, const bf16* x, const bf16* res, const float* scale, const float* shift,
                          const float* mean, const float* invstd, int M, int C, int act, float slope, float* partials,
                          float* out, hipStream_t s, int inv = 0);
// inv = 1: InplaceABN backward -- x is the layer OUTPUT y (act invertible: none / leaky), mean /
// invstd are beta / 1/gamma, and the pre-activation is recovered in registers
// dg != nullptr (with sums): also dg = sign(graw) * sums[1] -- InplaceABN's raw-weight gradient
void launch_bn_bwd_elemt(const bf16* dy, const bf16* x, const bf16* res, const float* scale, const float* shift,
                         const float* mean, const float* invstd, const float* sums, float inv_count, size_t numel,
                         int C, int act, float slope, bf16* dx, bf16* dres, hipStream_t s, int inv = 0,
                         const float* graw = nullptr, float* dg = nullptr);

void launch_maxpool_fwd(const bf16* x, bf16* y, uint8_t* idx, int N, int H, int W, int C, int Ho, int Wo, int k,
                        int s, int p, hipStream_t st, const float* scale = nullptr, const float* shift = nullptr,
                        int act = 0);
// backward of BN(+act) -> max pool: dx == nullptr -> reduction pass (part: maxpool_bn_bwd_blocks() x 2 x C
// scratch, sums_out [2][C]); else the elementwise pass with the global `sums`
int maxpool_bn_bwd_blocks();
void launch_maxpool_bn_bwd(const bf16* dy, const uint8_t* idx, const bf16* x, int N, int H, int W, int C, int Ho,
                           int Wo, int k, int s, int p, const float* scale, const float* shift, const float* mean,
                           const float* invstd, int act, float* part, float* sums_out, const float* sums,
                           float inv_count, bf16* dx, hipStream_t st);
void launch_maxpool_bwd(const bf16* dy, const uint8_t* idx, bf16* dx, int N, int H, int W, int C, int Ho, int Wo,
                        int k, int s, int p, hipStream_t st);
// two-level reductions over HW per (n, c) (gap_fwd, chan_scale_bwd): row splits S; the
// part workspace holds S x N x C floats
int hw_splits(int N, int HW, int C);
void launch_gap_fwd(const bf16* x, bf16* y, float* part, int N, int HW, int C, hipStream_t st);
void launch_gap_bwd(const bf16* dy, bf16* dx, int N, int HW, int C, hipStream_t st, const bf16* add = nullptr);
void launch_s2d(const bf16* x, bf16* y, int N, int H, int W, int C, int b, int inverse, hipStream_t st);

void launch_xent_fwd(const void* logits, bool is_bf16, int B, int ld, int C, const int64_t* labels, float* loss,
                     int* rank, float smoothing, hipStream_t s);
void launch_metric_accum(double* acc, const float* loss, int nloss, float loss_scale, const int* rank, int nrows,
                         hipStream_t s);
void launch_xent_bwd(const void* logits, bool in_bf16, int B, int ld, int C, const int64_t* labels,
                     const float* grad_out, float scale, float smoothing, void* dlogits, int ldo, bool out_bf16,
                     hipStream_t s);
// two-label (Mixup / CutMix) cross-entropy: row b carries labels[b] with weight wlab[b] and
// labels[partner[b]] with 1 - wlab[b]; rank is that of labels[b]
void launch_xent_mix_fwd(const void* logits, bool is_bf16, int B, int ld, int C, const int64_t* labels,
                         const int* partner, const float* wlab, float* loss, int* rank, float smoothing,
                         hipStream_t s);
void launch_xent_mix_bwd(const void* logits, bool in_bf16, int B, int ld, int C, const int64_t* labels,
                         const int* partner, const float* wlab, const float* grad_out, float scale, float smoothing,
                         void* dlogits, int ldo, bool out_bf16, hipStream_t s);
void launch_log_softmax_fwd(const void* x, bool is_bf16, int B, int ld, int C, float* y, hipStream_t s);
void launch_log_softmax_bwd(const float* y, const float* dy, int B, int C, int ldo, void* dx, bool out_bf16,
                            hipStream_t s);
void launch_l2norm_rows(const void* x, bool is_bf16, int R, int Rout, int D, int ldo, bf16* y, float* inv_norm, float eps,
                        hipStream_t s);
void launch_l2norm_bwd(const void* dy, bool dy_bf16, int ldd, const bf16* y, int ldy, const float* inv_norm, int R,
                       int D, void* dx, bool out_bf16, hipStream_t s);
void launch_transpose2d(const bf16* x, bf16* y, int R, int C, hipStream_t s);
void launch_arcface_fwd(const bf16* cosv, int B, int ld, int C, const int64_t* labels, float s, float cos_m,
                        float sin_m, float th, float mm, int easy, float* out_logits, float* loss, int* rank,
                        float* lab_dphi, hipStream_t st);
void launch_arcface_bwd(const bf16* cosv, int B, int ld, int C, const int64_t* labels, float s, float cos_m,
                        float sin_m, float th, float mm, int easy, const float* lab_dphi, const float* grad_out,
                        float scale, bf16* dcos, hipStream_t st);

struct MTEntry {
  float* p;
  float* g;
  float* s1;
  float* s2;
  bf16* shadow;
  int64_t n;
};
struct SgdHyper {
  float lr, momentum, dampening, wd, grad_scale;
  int nesterov, first;
};
// Device control block of global gradient-norm clipping (written by gnorm_finish, read by the update
// kernels): the step's coefficient, whether the step is skipped (non-finite norm), the norm, the
// running count of skipped steps, and the epoch that stamps this step's partials.  32 bytes.
struct ClipCtl {
  float coef;
  int skip;
  float norm;
  int skipped;
  unsigned epoch;
  int pad[3];
};
// One slot of the norm's partials: a chunk's sum of g^2 and the epoch of the step that wrote it.
struct GnormPartial {
  float sum;
  unsigned epoch;
};
struct AdamHyper {
  float lr, beta1, beta2, eps, wd, grad_scale, bc1, bc2;
  // 1 - beta and log(beta), formed in double from the caller's beta and then rounded: 1.f - (float)0.999
  // is 1.3e-5 off 1 - 0.999 (the second moment and, with logf of the rounded beta, the bias correction)
  float omb1, omb2, lb1, lb2;
  int decoupled;
  const int* step_dev;  // optional device step count: bc1/bc2 computed in-kernel from it
  const float* lr_dev;  // optional device learning rate, read by the kernel instead of lr
  const ClipCtl* clip;  // optional: grad_scale becomes fl(grad_scale * coef); a set skip flag writes nothing
};
struct LarsHyper {
  SgdHyper sgd;         // wd and grad_scale enter the scaled gradient d; the SGD update on d has no decay
  const float* trust;   // per table entry, or null: every trust ratio is 1 (a non-adaptive group)
  const float* lr_dev;  // optional device learning rate, read by the kernel instead of sgd.lr
  const ClipCtl* clip;  // optional, as in AdamHyper
  int trust_clip;       // LARC's clip mode: trust <- min(trust / lr, 1), 1 when lr <= 0
};
struct LambHyper {
  float lr, beta1, beta2, eps, wd, grad_scale;
  float bc1, bc2;          // 1 - beta^step from the host (1 without bias correction); replaced in-kernel
  float omb1, omb2, lb1, lb2;  // as in AdamHyper
  int bias_correction;
  const int* step_dev;     // optional device step count (bias corrections of a replayed HIP graph)
  const float* lr_dev;     // optional device learning rate
  const float* trust;      // per table entry; set by launch_mt_lamb
  const ClipCtl* clip;     // optional, as in AdamHyper
  float phi_min, phi_max;  // trust = clamp(|w|, phi_min, phi_max) / |u|; 0 and +inf: |w| / |u|
};
// Global gradient norm.  launch_mt_gnorm2: per-chunk sums of g^2 of the table's tensors into
// partials[slots[entry] + chunk], stamped with ctl's epoch.  launch_gnorm_finish: all nslots slots
// (each weighted with slot_gs^2, its group's grad_scale) merged into ctl's norm, coefficient
// (max_norm > 0, else 1) and skip flag (skip_nonfinite and a non-finite norm).
void launch_mt_gnorm2(const MTEntry* tab, const int2* chunks, int nchunks, const int* slots, const ClipCtl* ctl,
                      GnormPartial* partials, hipStream_t s);
void launch_gnorm_finish(const GnormPartial* partials, int nslots, const float* slot_gs, float max_norm,
                         int skip_nonfinite, ClipCtl* ctl, hipStream_t s);
// mode: bit 0 = source bf16, bit 1 = destination bf16 (MTEntry.p = destination, .g = source)
void launch_mt_copy(const MTEntry* tab, const int2* chunks, int nchunks, float scale, int mode, hipStream_t s);
// Weight EMA (MTEntry.p = live tensor, .s1 = its average): e = fma(*omd_dev, p - e, e) per element,
// nothing written when ctl (optional) has its skip flag set; and the in-place exchange of p and s1.
void launch_mt_ema(const MTEntry* tab, const int2* chunks, int nchunks, const float* omd_dev, const ClipCtl* ctl,
                   hipStream_t s);
void launch_mt_swap(const MTEntry* tab, const int2* chunks, int nchunks, hipStream_t s);
void launch_mt_sgd(const MTEntry* tab, const int2* chunks, int nchunks, SgdHyper h, hipStream_t s);
void launch_mt_adam(const MTEntry* tab, const int2* chunks, int nchunks, AdamHyper h, hipStream_t s);
// LARS step: per-chunk sums of squares into partials [nchunks], per-tensor trust ratios (spans
// [ntensors] = (first chunk, chunk count)) into trust [ntensors], then the update.  trust == null:
// the two norm launches are skipped and every ratio is 1.
void launch_mt_lars(const MTEntry* tab, const int2* chunks, int nchunks, const int2* spans, int ntensors,
                    float2* partials, float* trust, float eta, float eps, LarsHyper h, hipStream_t s);
// LAMB step.  trust != null: moments + per-chunk (sum w^2, sum u^2) into partials [nchunks], per-tensor
// trust ratios |w| / |u| into trust [ntensors], then the update.  trust == null (a non-adaptive group):
// one launch, the moments kernel applies the update itself with every ratio 1.
void launch_mt_lamb(const MTEntry* tab, const int2* chunks, int nchunks, const int2* spans, int ntensors,
                    float2* partials, float* trust, LambHyper h, hipStream_t s);
void launch_cdr_threshold(const MTEntry* tab, const int2* chunks, int nchunks, uint32_t* state, uint32_t* hist,
                          hipStream_t s);
void launch_cdr_mask(const MTEntry* tab, const int2* chunks, int nchunks, const uint32_t* state, float clip,
                     hipStream_t s);

// local training BN: statistics finalize (from conv slabs [R][2][C], R <= bn_direct_slabs(), or
// partials [P][3][C]) + BN / act (+ residual, + mask bits) in one launch; sync: 3 zeroed uint32 counters
// reserved for this stream (re-armed by every launch; sync[2] != 0 after a spin timeout)
int bn_direct_slabs();
void launch_bn_fin_act(const bf16* x, const bf16* res, const float* src, int nsrc, int partials, int M, int C,
                       float eps, const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                       float* shift, float* rm, float* rv, float momentum, float iabn_eps, float* rgamma, bf16* y,
                       uint8_t* mask, int act, float slope, uint32_t* sync, hipStream_t s);

// direct 3x3 / s1 / p1 conv, 64 -> 64 channels (conv3x3.hip); part: [blocks][3][64] (n, mean, M2) or null
bool conv3x3_c64_supported(int H, int W, int C, int Co);
int conv3x3_c64_blocks(int N, int H, int W, int num_cu);
void launch_conv3x3_c64(const bf16* x, const bf16* w, bf16* y, float* part, const bf16* zero, int N, int H, int W,
                        int blocks, hipStream_t stream, const float* pscale = nullptr, const float* pshift = nullptr,
                        int wflip = 0);

// host int64 table -> device through kernel arguments (graph-capture safe, see misc.hip)
void launch_table_fill(const int64_t* host, int64_t n, int64_t* out, hipStream_t s);
void launch_weight_prep(const float* w, int Co, int T, int Ci, int Co_pad, bf16* wb, bf16* wt, hipStream_t s);
// entries: packed {w, wb, wt, Co, T, Ci_src, Ci, Cp, tci, tco, pad} (56 B each); blocks: int2 (entry, tile)
void launch_mt_weight_prep(const void* entries, const void* blocks, int nblocks, hipStream_t s);
void launch_to_nhwc(const void* src, int is_u8, int nchw, int N, int C, int H, int W, int Cp, float in_scale,
                    const float* mean, const float* stdv, bf16* dst, hipStream_t s);
// space-to-depth input: block 2 (ResNet s2d stem) dst [N][H/2][W/2][16], channel (py*2+px)*4 + c (c < 3
// real); block 4 (TResNet SpaceToDepth(4)) dst [N][H/4][W/4][48], channel (py*4+px)*3 + c
void launch_to_nhwc_s2d(const void* src, int is_u8, int nchw, int N, int C, int H, int W, float in_scale,
                        const float* mean, const float* stdv, bf16* dst, hipStream_t s, int block = 2);
// Mixup / CutMix while normalising: row n mixed with row partner[n] by blend[n] outside box[n] = {y0, x0, y1, x1}
// and replaced by it inside (misc.hip).  block 0: the plain [N][H][W][8] layout; 2 / 4: as launch_to_nhwc_s2d.
// Returns 1 (nothing launched) when the output pixels exceed the 32-bit index range.
int launch_to_nhwc_mix(const void* src, int is_u8, int nchw, int N, int C, int H, int W, float in_scale,
                       const float* mean, const float* stdv, const int* partner, const float* blend, const int* box,
                       bf16* dst, hipStream_t s, int block);
// shard-loader augmentation: meta [B][8] = {byte offset, H, W, y0, x0, h, w, flip} -> out [B][Ho][Wo][3]
void launch_crop_resize(const uint8_t* src, const int64_t* meta, int B, int Ho, int Wo, uint8_t* out, hipStream_t s);
// the same with a per-image inverse affine map xf [B][8] = {m00, m01, m02, m10, m11, m12, angle_deg, 0}
// (output pixel -> box-relative source position) and fill 0 outside the box
void launch_warp_crop(const uint8_t* src, const int64_t* meta, const float* xf, int B, int Ho, int Wo, uint8_t* out,
                      hipStream_t s);
// PIL-exact resampling (the loader's `pil` mode): Pillow's two-pass fixed-point resize of each box
// to its canvas, then the (mirrored-first) Ho x Wo window; geo [B][12] = {Sh, Sw, dy, dx, a0..a5,
// rotate, angle bits}.  hmeta / hgeo are the HOST copies the refusals are decided from; the return
// value is 0 or a refusal code with the image in *bad (resample_check in augment.hip), nothing is launched then.
int launch_resample_crop(const uint8_t* src, const int64_t* meta, const int32_t* geo, const int64_t* hmeta,
                         const int32_t* hgeo, int B, int Ho, int Wo, int bicubic, int whole, uint8_t* out, int* bad,
                         hipStream_t s);
// Image.rotate(NEAREST) through geo's 16.16 integers -> mirror -> window, of canvases [B][Sh][Sw][3]
int launch_rotate_nearest_crop(const uint8_t* canvas, const int64_t* meta, const int32_t* geo, const int32_t* hgeo,
                               int B, int Sh, int Sw, int Ho, int Wo, uint8_t* out, int* bad, hipStream_t s);
void launch_act_bwd(const bf16* dy, const bf16* y, bf16* dx, size_t numel, int act, hipStream_t s);
void launch_prefix_mask(const bf16* x, bf16* y, int B, int D, const int* keep, hipStream_t s);
// InplaceABN effective weight: geff = |g| + eps, rg = 1 / geff; backward out = d * sign(g)
void launch_iabn_gamma(const float* g, float eps, float* geff, float* rg, int C, hipStream_t s);
void launch_sign_mul(const float* d, const float* g, float* out, int C, hipStream_t s);
// Philox dropout (misc.hip): y = x * keep / (1 - p); keep from (seed, *offset_ptr, element index);
// `used` (optional) receives the offset the launch drew with (for the mask-regenerating backward)
void launch_dropout(const void* x, void* y, size_t n, int is_bf16, float p, uint64_t seed, const int64_t* offset_ptr,
                    int64_t* used, hipStream_t s);
// adaptive average pool NHWC [N,H,W,C] -> [N,OH,OW,C]; backward = true: dy [N,OH,OW,C] -> dx [N,H,W,C]
void launch_adaptive_avg(const bf16* src, bf16* dst, int N, int H, int W, int C, int OH, int OW, bool backward,
                         hipStream_t s);
void launch_nested_eval_scalar(const float* feat, const float* W, const int64_t* labels, int B, int D, int C,
                               int* counts, hipStream_t s);
// weight-stationary persistent 1x1 stride-1 forward GEMM (conv_ws.hip): src [M][K], wt [Co][ldw] -> dst [M][Co]
// (+ per-128-row slab BN statistics); K in {64, 128, 256}, Co % 128 == 0; false = unsupported
bool conv1x1_ws_supported(int K, int Co, long M);
bool launch_conv1x1_ws(const bf16* src, const bf16* wt, int ldw, bf16* dst, float* stats, const bf16* zero, int M,
                       int K, int Co, hipStream_t st);
// store-decoupled persistent 1x1 stride-1 forward GEMM (conv1x1_ps.hip): loader waves fill an LDS-DMA
// ring, consumer waves store straight from the accumulators; same contract as launch_conv1x1_ws
// (ablate: conv1x1_ps.hip PsParams; timing experiments only); cw: consumer waves, 4 or 8
bool conv1x1_ps_supported(int K, int Co, long M);
bool launch_conv1x1_ps(const bf16* src, const bf16* wt, int ldw, bf16* dst, float* stats, const bf16* zero, int M,
                       int K, int Co, int ablate, int cw, hipStream_t st);
// Fused ArcFace head (arcface.hip): no [B, C] tensor.  xn [Bp][Dp] / wn [Cp][Dp] normalised bf16
// (zero padding rows), Bp % 64 == Cp % 64 == 0, Dp in {128, 256, 512}, any batch size (the kernels'
// LDS does not depend on it); false = unsupported shape.  The partial buffers follow the *_splits
// functions: part [S][Bp][4] (fwd), [S][Bp][Dp] (dx), [S][Cp][Dp] (dw, S > 1); info [Bp][4] is the
// dW kernel's per-row scratch.
bool launch_arcface_l2norm_t(const void* x, bool is_bf16, int R, int D, int Rp, int Dp, bf16* y, bf16* yT, float* inv,
                             float eps, hipStream_t st);
int arcface_fused_fwd_splits(int Bp, int Cp);
int arcface_fused_dx_splits(int Bp, int Cp);
bool launch_arcface_fused_fwd(const bf16* xn, const bf16* wn, const int64_t* labels, int B, int Bp, int C, int Cp,
                              int Dp, float s, float m, int easy, float* lab, float* part, float* loss, int* rank,
                              float* lse, hipStream_t st);
bool launch_arcface_fused_dx(const bf16* xn, const bf16* wn, const bf16* wnT, const int64_t* labels, int B, int Bp,
                             int C, int Cp, int Dp, int D, float s, const float* lab, const float* lse,
                             const float* gout, float scale, const float* inv_x, float* part, void* dx, bool dx_bf16,
                             hipStream_t st);
int arcface_fused_dw_splits(int Bp, int Cp);
bool launch_arcface_fused_dw(const bf16* xn, const bf16* xnT, const bf16* wn, const int64_t* labels, int B, int Bp,
                             int C, int Cp, int Dp, int D, float s, const float* lab, const float* lse,
                             const float* gout, float scale, const float* inv_w, float* part, float* info,
                             float* dw, hipStream_t st);
// SyncBN peer-memory exchange (peer.hip): gather (mode 0, dst [world][n]) or rank-ordered sum
// (mode 1, dst [n]) of n floats through the IPC-mapped mailboxes `boxes` ([world] base addresses);
// a rank missing for timeout_ms sets *err and poisons dst with NaN (this and every later exchange)
bool launch_peer_exchange(const float* src, int n, float* dst, const int64_t* boxes, int* epoch, int rank, int world,
                          int slot, int mode, int* err, int timeout_ms, hipStream_t s);
// workspace bytes of launch_nested_eval (label score chains + per-class-block rank counts)
size_t nested_eval_workspace(int B, int D, int C);
void launch_nested_eval(const float* feat, const float* W, const int64_t* labels, int B, int D, int C, int* counts,
                        void* ws, hipStream_t s);

void launch_dwconv_fwd(const bf16* x, const float* w, bf16* y, int N, int H, int W, int C, int Ho, int Wo, int k,
                       int s, int p, int reflect, hipStream_t st);
void launch_dwconv_bwd(const bf16* dy, const float* w, bf16* dx, int N, int H, int W, int C, int Ho, int Wo, int k,
                       int s, int p, int reflect, hipStream_t st);
void launch_chan_scale_fwd(const bf16* x, const bf16* g, const bf16* res, bf16* y, int N, int HW, int C, int relu,
                           hipStream_t st);
// squeeze-excitation gate of a small batch, one MFMA workgroup per direction (extra.hip): p [N,C],
// W1 [>=R rows, C], W2 [>=C rows, R] bf16 forward; their transposes W1^T [C][ld1t], W2^T [R][ld2t] backward
bool se_gate_supported(int N, int C, int R);
void launch_se_gate_fwd(const bf16* p, const bf16* w1, const float* b1, const bf16* w2, const float* b2, bf16* h,
                        bf16* g, int N, int C, int R, hipStream_t st);
void launch_se_gate_bwd(const bf16* dg, const bf16* g, const bf16* h, const bf16* p, const bf16* w1t, int ld1t,
                        const bf16* w2t, int ld2t, float* dw1, float* db1, float* dw2, float* db2, bf16* dp, int N,
                        int C, int R, hipStream_t st);
void launch_chan_scale_bwd(const bf16* dy, const bf16* x, const bf16* g, const bf16* res, bf16* dx, bf16* dg, float* part,
                           bf16* dres, int N, int HW, int C, int relu, hipStream_t st);

// stem weight 7x7/2 [Co][7][7][C<=4] <-> space-to-depth 4x4 [Co][4][4][16] (misc.hip)
void launch_s2d_weight(const float* w7, int Co, int C, float* w16, hipStream_t s);
void launch_s2d_weight_bwd(const float* g16, int Co, int C, float* g7, hipStream_t s);

}  // namespace dcp
