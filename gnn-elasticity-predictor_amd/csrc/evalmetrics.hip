// evalmetrics.hip — the validation epoch's metrics on the device ("Validation epoch").
//
// eval_epoch_hetero (train.py:726-846) reads nine or more device values per batch on the host and
// ranks the collected |error| / sigma with SciPy at the end.  Here one launch per batch folds the
// batch into a small block of doubles and appends |y_z - mean| and max(sigma, 1e-6) to two epoch
// buffers; at the end of the epoch a counting rank (tie-exact, no sort) and a Pearson correlation
// of the ranks give Spearman, and one thread forms the nine outputs with the reference's
// denominators.  No atomics anywhere: every sum is taken in a fixed order, so two runs are bitwise
// equal.
//
// Per element, in the reference's fp32 operation order (bf16 heads are widened first):
//   lv = max(logvar, floor); var = exp(lv); sigma = sqrt(var)
//   y_z = (log y - m) / s           (LogTransformer.transform_tensor; no transformer: y_z = y)
//   d = mean - y_z; nll = 0.5 (lv + d^2 / var)
//   pred = exp(mean * s + m)        (two roundings, as torch's mul then add; no transformer: mean)
//   |pred - y|, (pred - y)^2, |log max(pred, 1e-6) - log max(y, 1e-6)|
#include <math.h>

#include "common.h"

namespace alignn {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / ALIGNN_WAVE;
constexpr int kEvalLevels = ALIGNN_EVAL_LEVELS;
constexpr int kRankTile = ALIGNN_EVAL_RANK_TILE;  // floats of x staged in LDS per pass (4 KiB)

// per-thread partial sums of the batch kernel (counts are exact in double)
enum { P_NLL = 0, P_LV, P_ABS, P_SQ, P_LOGABS, P_HITS, P_BAD, P_ECE, P_COUNT = P_ECE + kEvalLevels };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// max that keeps a NaN, as torch.max does
__device__ __forceinline__ float wave_max_nan(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __builtin_elementwise_maximum(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }

template <typename H>
__global__ __launch_bounds__(kEvalThreads) void eval_accumulate_kernel(
    int64_t B, int T, const H* __restrict__ heads, int64_t ldh, const float* __restrict__ y,
    const float* __restrict__ lm, const float* __restrict__ ls, float floor_lv, const float* __restrict__ zth,
    const float* __restrict__ plev, int log_mae, double* __restrict__ state, float* __restrict__ err_buf,
    float* __restrict__ sig_buf, int64_t cap) {
  __shared__ double red[kEvalWaves][P_COUNT];
  __shared__ float redmax[kEvalWaves];
  const int64_t total = B * T;
  const int64_t cur = (int64_t)state[ALIGNN_EVAL_S_CURSOR];  // read by all before thread 0 advances it (barrier below)
  float z[kEvalLevels];
#pragma unroll
  for (int l = 0; l < kEvalLevels; ++l) z[l] = zth[l];
  double p[P_COUNT];
#pragma unroll
  for (int k = 0; k < P_COUNT; ++k) p[k] = 0.0;
  float smax = -INFINITY;
  for (int64_t i = threadIdx.x; i < total; i += kEvalThreads) {
    const int64_t b = i / T;
    const int t = (int)(i - b * T);
    const float yv = y[i];
    const int64_t slot = cur + i;
    if (lm && yv <= 0.f) {
      // transform_tensor raises on such a batch; here it is counted and the host raises at the end
      // of the epoch.  The element adds to no sum; its buffer slots are masked out of Spearman.
      p[P_BAD] += 1.0;
      if (slot < cap) {
        err_buf[slot] = NAN;
        sig_buf[slot] = NAN;
      }
      continue;
    }
    const float mean = (float)heads[b * ldh + t];
    const float lv = clamp_min((float)heads[b * ldh + T + t], floor_lv);
    const float var = expf(lv);
    const float sigma = sqrtf(var);
    float yz = yv, pred = mean;
    if (lm) {
      const float m = lm[t], s = ls[t];
      yz = (logf(yv) - m) / s;
      pred = expf(__fadd_rn(__fmul_rn(mean, s), m));
    }
    const float d = mean - yz;
    const float ad = fabsf(d);
    p[P_NLL] += (double)(0.5f * (lv + d * d / var));
    p[P_LV] += (double)lv;
    const float e = pred - yv;
    p[P_ABS] += (double)fabsf(e);
    p[P_SQ] += (double)(e * e);
    if (log_mae) p[P_LOGABS] += (double)fabsf(logf(clamp_min(pred, 1e-6f)) - logf(clamp_min(yv, 1e-6f)));
    if (ad <= sigma) p[P_HITS] += 1.0;
#pragma unroll
    for (int l = 0; l < kEvalLevels; ++l)
      if (ad <= z[l] * sigma) p[P_ECE + l] += 1.0;
    smax = __builtin_elementwise_maximum(smax, sigma);
    if (slot < cap) {
      err_buf[slot] = ad;
      sig_buf[slot] = clamp_min(sigma, 1e-6f);
    }
  }
  const int lane = threadIdx.x & 63, w = wave_id();
#pragma unroll
  for (int k = 0; k < P_COUNT; ++k) {
    const double v = wave_sum_d(p[k]);
    if (lane == 0) red[w][k] = v;
  }
  smax = wave_max_nan(smax);
  if (lane == 0) redmax[w] = smax;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot[P_COUNT];
  for (int k = 0; k < P_COUNT; ++k) {
    double v = red[0][k];
    for (int q = 1; q < kEvalWaves; ++q) v += red[q][k];
    tot[k] = v;
  }
  float bmax = redmax[0];
  for (int q = 1; q < kEvalWaves; ++q) bmax = __builtin_elementwise_maximum(bmax, redmax[q]);
  const double n = (double)total;
  state[ALIGNN_EVAL_S_LOSS] += tot[P_NLL] / (double)T;  // sum over graphs of the mean over targets
  state[ALIGNN_EVAL_S_GRAPHS] += (double)B;
  state[ALIGNN_EVAL_S_LV_SUM] += tot[P_LV];
  state[ALIGNN_EVAL_S_LV_COUNT] += n;
  // Python's max(prev, batch_max): a NaN batch maximum compares false and is dropped (train.py:782)
  if ((double)bmax > state[ALIGNN_EVAL_S_SIGMA_MAX]) state[ALIGNN_EVAL_S_SIGMA_MAX] = (double)bmax;
  state[ALIGNN_EVAL_S_COV_HITS] += tot[P_HITS];
  state[ALIGNN_EVAL_S_ELEMS] += n;
  // ECE per batch (train.py:803-807): fp32 coverage of this batch at each level against the fp32
  // level, the nine terms added once per batch whatever its size
  double ece = 0.0;
  for (int l = 0; l < kEvalLevels; ++l) {
    const float cov = (float)tot[P_ECE + l] / (float)total;
    ece += (double)fabsf(cov - plev[l]);
  }
  state[ALIGNN_EVAL_S_ECE_SUM] += ece;
  state[ALIGNN_EVAL_S_ECE_TERMS] += (double)kEvalLevels;
  state[ALIGNN_EVAL_S_ABS] += tot[P_ABS];
  state[ALIGNN_EVAL_S_SQ] += tot[P_SQ];
  state[ALIGNN_EVAL_S_LOGABS] += tot[P_LOGABS];
  state[ALIGNN_EVAL_S_BAD] += tot[P_BAD];
  state[ALIGNN_EVAL_S_CURSOR] += n;
}

// ---------------------------------------------------------------------------------------------
// Spearman with average ranks.  Workspace (doubles): [0] m = number of pairs with both values
// finite, [1] unused, [2, 2+n) ranks of err, [2+n, 2+2n) ranks of sig, then 2n floats: the compacted
// err and sig.
// ---------------------------------------------------------------------------------------------

// Order-preserving compaction by one workgroup: ballot + popcount inside a wave, wave totals in LDS.
__global__ __launch_bounds__(kEvalThreads) void eval_compact_kernel(int64_t n, const float* __restrict__ err,
                                                                    const float* __restrict__ sig,
                                                                    float* __restrict__ cx, float* __restrict__ cs,
                                                                    double* __restrict__ count) {
  __shared__ int wtot[kEvalWaves];
  const int lane = threadIdx.x & 63, w = wave_id();
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kEvalThreads) {
    const int64_t i = c0 + threadIdx.x;
    float a = 0.f, b = 0.f;
    bool ok = false;
    if (i < n) {
      a = err[i];
      b = sig[i];
      ok = finite_f(a) && finite_f(b);
    }
    const unsigned long long mask = __ballot(ok);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(mask);
    __syncthreads();
    int off = 0, chunk = 0;
    for (int q = 0; q < kEvalWaves; ++q) {
      if (q < w) off += wtot[q];
      chunk += wtot[q];
    }
    if (ok) {
      cx[base + off + pre] = a;
      cs[base + off + pre] = b;
    }
    base += chunk;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  if (threadIdx.x == 0) *count = (double)base;
}

// rank_i = #(x_j < x_i) + (#(x_j == x_i) + 1) / 2 by counting: x streams through LDS in tiles, each
// thread keeps its own x_i in a register and every lane reads the same LDS address (a broadcast, no
// bank conflicts).  The tile's tail is padded with NaN, which compares false both ways.
// blockIdx.y picks the array.
__global__ __launch_bounds__(kEvalThreads) void eval_rank_kernel(int64_t n, const double* __restrict__ count,
                                                                 const float* __restrict__ cx,
                                                                 const float* __restrict__ cs,
                                                                 double* __restrict__ rx, double* __restrict__ rs) {
  __shared__ __attribute__((aligned(16))) float tile[kRankTile];
  int64_t m = (int64_t)*count;
  if (m > n) m = n;
  const int64_t i0 = (int64_t)blockIdx.x * kEvalThreads;
  if (i0 >= m) return;  // whole workgroup: the grid is sized from n, the finite count is known on the device only
  const float* __restrict__ x = blockIdx.y ? cs : cx;
  double* __restrict__ r = blockIdx.y ? rs : rx;
  const int64_t i = i0 + threadIdx.x;
  const float xi = i < m ? x[i] : 0.f;
  int less = 0, eq = 0;
  for (int64_t t0 = 0; t0 < m; t0 += kRankTile) {
#pragma unroll
    for (int k = 0; k < kRankTile / kEvalThreads; ++k) {
      const int64_t j = t0 + k * kEvalThreads + threadIdx.x;
      tile[k * kEvalThreads + threadIdx.x] = j < m ? x[j] : NAN;
    }
    __syncthreads();
    const float4* t4 = reinterpret_cast<const float4*>(tile);
#pragma unroll 8
    for (int q = 0; q < kRankTile / 4; ++q) {
      const float4 v = t4[q];
      less += (int)(v.x < xi) + (int)(v.y < xi) + (int)(v.z < xi) + (int)(v.w < xi);
      eq += (int)(v.x == xi) + (int)(v.y == xi) + (int)(v.z == xi) + (int)(v.w == xi);
    }
    __syncthreads();
  }
  if (i < m) r[i] = (double)less + 0.5 * (double)(eq + 1);  // eq counts x_i itself
}

// Pearson correlation of the two rank vectors in double.  Average ranks always have mean (m+1)/2,
// and the centred ranks are multiples of 0.5, so the three sums are exact for any m a counting
// rank can serve.  Fewer than two pairs or a constant vector: NaN (SciPy's answer).
__global__ __launch_bounds__(kEvalThreads) void eval_rank_corr_kernel(int64_t n, const double* __restrict__ count,
                                                                      const double* __restrict__ rx,
                                                                      const double* __restrict__ rs,
                                                                      double* __restrict__ out) {
  __shared__ double red[kEvalWaves][3];
  int64_t m = (int64_t)*count;
  if (m > n) m = n;
  const double mu = 0.5 * (double)(m + 1);
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kEvalThreads) {
    const double a = rx[i] - mu, b = rs[i] - mu;
    sxy += a * b;
    sxx += a * a;
    syy += b * b;
  }
  sxy = wave_sum_d(sxy);
  sxx = wave_sum_d(sxx);
  syy = wave_sum_d(syy);
  const int lane = threadIdx.x & 63, w = wave_id();
  if (lane == 0) {
    red[w][0] = sxy;
    red[w][1] = sxx;
    red[w][2] = syy;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[3];
  for (int k = 0; k < 3; ++k) {
    double v = red[0][k];
    for (int q = 1; q < kEvalWaves; ++q) v += red[q][k];
    t[k] = v;
  }
  double rho = NAN;
  if (m >= 2 && t[1] > 0.0 && t[2] > 0.0) {
    rho = t[0] / sqrt(t[1] * t[2]);
    rho = fmin(fmax(rho, -1.0), 1.0);
  }
  *out = rho;
}

// The nine outputs with the reference's denominators and empty-epoch values (train.py:823-845);
// out[9] is the non-positive-target count for the host's ValueError.
__global__ void eval_finalize_kernel(const double* __restrict__ state, int64_t dataset_size,
                                     const double* __restrict__ spearman, int log_mae, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double graphs = state[ALIGNN_EVAL_S_GRAPHS], elems = state[ALIGNN_EVAL_S_ELEMS];
  const double ds = (double)dataset_size;
  out[0] = graphs > 0.0 ? state[ALIGNN_EVAL_S_LOSS] / graphs : 0.0;
  out[1] = dataset_size > 0 ? state[ALIGNN_EVAL_S_ABS] / ds : 0.0;  // by dataset_size, not by elements (train.py:827)
  out[2] = (dataset_size > 0 && log_mae) ? state[ALIGNN_EVAL_S_LOGABS] / ds : (double)NAN;
  out[3] = elems > 0.0 ? sqrt(state[ALIGNN_EVAL_S_SQ] / elems) : (double)NAN;
  out[4] = spearman ? *spearman : (double)NAN;
  out[5] = state[ALIGNN_EVAL_S_LV_COUNT] > 0.0 ? state[ALIGNN_EVAL_S_LV_SUM] / state[ALIGNN_EVAL_S_LV_COUNT] : (double)NAN;
  out[6] = state[ALIGNN_EVAL_S_SIGMA_MAX] > -INFINITY ? state[ALIGNN_EVAL_S_SIGMA_MAX] : (double)NAN;
  out[7] = elems > 0.0 ? state[ALIGNN_EVAL_S_COV_HITS] / elems : (double)NAN;
  out[8] = state[ALIGNN_EVAL_S_ECE_TERMS] > 0.0 ? state[ALIGNN_EVAL_S_ECE_SUM] / state[ALIGNN_EVAL_S_ECE_TERMS] : (double)NAN;
  out[9] = state[ALIGNN_EVAL_S_BAD];
}

}  // namespace alignn

using namespace alignn;

extern "C" int alignn_eval_accumulate(int64_t B, int32_t T, const void* heads, int32_t heads_bf16, int64_t ldh,
                                      const float* y, const float* log_means, const float* log_stds,
                                      float min_logvar_floor, const float* z_thresholds, const float* prob_levels,
                                      int32_t compute_log_mae, double* state, float* err_buf, float* sig_buf,
                                      int64_t capacity, void* stream) {
  if (B < 0 || T < 1 || ldh < 2 * (int64_t)T || capacity < 0) {
    set_error("eval_accumulate: need B >= 0, T >= 1, ldh >= 2T, capacity >= 0 (B=%lld T=%d ldh=%lld capacity=%lld)",
              (long long)B, T, (long long)ldh, (long long)capacity);
    return ALIGNN_E_BAD_SHAPE;
  }
  if ((log_means == nullptr) != (log_stds == nullptr)) {
    set_error("eval_accumulate: log_means and log_stds go together");
    return ALIGNN_E_BAD_SHAPE;
  }
  if (B == 0) return ALIGNN_OK;
  if (!heads || !y || !z_thresholds || !prob_levels || !state || (capacity > 0 && (!err_buf || !sig_buf))) {
    set_error("eval_accumulate: null pointer");
    return ALIGNN_E_BAD_SHAPE;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (heads_bf16) {
    launch(eval_accumulate_kernel<__bf16>, dim3(1), dim3(kEvalThreads), 0, s, B, T, (const __bf16*)heads, ldh, y,
           log_means, log_stds, min_logvar_floor, z_thresholds, prob_levels, compute_log_mae, state, err_buf, sig_buf,
           capacity);
  } else {
    launch(eval_accumulate_kernel<float>, dim3(1), dim3(kEvalThreads), 0, s, B, T, (const float*)heads, ldh, y,
           log_means, log_stds, min_logvar_floor, z_thresholds, prob_levels, compute_log_mae, state, err_buf, sig_buf,
           capacity);
  }
  ALIGNN_LAUNCH_CHECK("eval_accumulate_kernel");
  return ALIGNN_OK;
}

extern "C" int alignn_eval_spearman(int64_t n, const float* err, const float* sig, double* out, double* workspace,
                                    void* stream) {
  if (n < 0 || n > ALIGNN_EVAL_SPEARMAN_MAX_N) {
    set_error("eval_spearman: n = %lld outside [0, %lld]", (long long)n, (long long)ALIGNN_EVAL_SPEARMAN_MAX_N);
    return ALIGNN_E_BAD_SHAPE;
  }
  if (!out || !workspace || (n > 0 && (!err || !sig))) {
    set_error("eval_spearman: null pointer");
    return ALIGNN_E_BAD_SHAPE;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* count = workspace;
  double* rx = workspace + 2;
  double* rs = rx + n;
  float* cx = reinterpret_cast<float*>(rs + n);
  float* cs = cx + n;
  launch(eval_compact_kernel, dim3(1), dim3(kEvalThreads), 0, s, n, err, sig, cx, cs, count);
  ALIGNN_LAUNCH_CHECK("eval_compact_kernel");
  if (n > 0) {
    launch(eval_rank_kernel, dim3((unsigned)((n + kEvalThreads - 1) / kEvalThreads), 2), dim3(kEvalThreads), 0, s, n,
           count, cx, cs, rx, rs);
    ALIGNN_LAUNCH_CHECK("eval_rank_kernel");
  }
  launch(eval_rank_corr_kernel, dim3(1), dim3(kEvalThreads), 0, s, n, count, rx, rs, out);
  ALIGNN_LAUNCH_CHECK("eval_rank_corr_kernel");
  return ALIGNN_OK;
}

extern "C" int alignn_eval_finalize(const double* state, int64_t dataset_size, const double* spearman,
                                    int32_t compute_log_mae, double* out, void* stream) {
  if (!state || !out) {
    set_error("eval_finalize: null pointer");
    return ALIGNN_E_BAD_SHAPE;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  launch(eval_finalize_kernel, dim3(1), dim3(ALIGNN_WAVE), 0, s, state, dataset_size, spearman, compute_log_mae, out);
  ALIGNN_LAUNCH_CHECK("eval_finalize_kernel");
  return ALIGNN_OK;
}
