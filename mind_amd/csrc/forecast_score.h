// Forecast scoring, one text for the two scoring kernels (k_forecast_modes, k_forecast_scenes: forecast_kernels.hip) and the host entry
// mind_debug_forecast_score: displacement errors of a K-mode forecast against a recorded future (minADE / minFDE / Brier-minFDE / miss
// rate) and the coverage of the discs the planner's exo term prices (radius max(sx, sy) + w_exo_cov_offset around the predicted mean,
// trajectory_tree.py:95-102, scenario_tree.py:325).
//
// Reference: the planner carries reg [a,6,60,5] = (x, y, sx, sy, exp rho) per agent in the agent-local frame (network.py:545) and never
// compares it with what the agents went on to do; the definitions below are the usual ones of motion forecasting and this project's.
//
// The order of operations is the contract (tests/forecast_restate.py restates it in numpy, operation for operation):
//  - forecast values are float32 and are converted to double FIRST; everything after is float64, no fma() here, and the including file
//    compiles with floating-point contraction off;
//  - every sum is sequential, in ascending t (per mode) or ascending agent index (per scene), from 0.0;
//  - every arg-minimum is the plain C loop `best = +inf, k = -1; for k ascending: if (v < best) take it`: the lowest k wins ties, a NaN never
//    wins, all modes NaN or +inf give -1;
//  - a non-finite forecast value has no special case: the arithmetic and the comparisons decide (`d <= r` is false for a NaN d, so
//    first_out names that sample; NaN sums propagate into ade / fde, which then lose every arg-minimum; NaN > miss_radius is no miss);
//  - the NaN of an empty set (no valid sample, no scored agent, no chosen mode) is FS_NAN.
// Samples: horizon h covers the samples t < horizon[h]; only samples with valid[t] != 0 count.
#pragma once

#if defined(__HIPCC__)
#define FS_FN __host__ __device__ __forceinline__
#else
#define FS_FN static inline
#endif

#define FS_MAX_K 8
#define FS_MAX_T 256
#define FS_MAX_H 4
#define FS_NAN __builtin_nan("")
#define FS_INF __builtin_inf()

typedef struct {
  int K, T, n_h;
  int horizon[FS_MAX_H];
  double miss_radius, disc_scale, disc_offset;
} fs_cfg;

// One sample: r4 = (x, y, sx, sy) of the forecast, (gx, gy) the truth.  d = the displacement, *inside = d <= r for the disc radius
// r = disc_scale * max(sx, sy) + disc_offset.
FS_FN double fs_sample(const float *r4, double gx, double gy, double disc_scale, double disc_offset, int *inside) {
  const double dx = (double)r4[0] - gx;
  const double dy = (double)r4[1] - gy;
  const double d = sqrt(dx * dx + dy * dy);
  const double r = disc_scale * (double)fmaxf(r4[2], r4[3]) + disc_offset;
  *inside = d <= r ? 1 : 0;
  return d;
}

// The running state of one (agent, mode) over its valid samples in ascending t
typedef struct {
  double sum, d_last;
  int n, last, cover, first_out;
} fs_run;

FS_FN void fs_run_init(fs_run *r) {
  r->sum = 0.0; r->d_last = FS_NAN;
  r->n = 0; r->last = -1; r->cover = 0; r->first_out = -1;
}
// a VALID sample t with displacement d
FS_FN void fs_run_step(fs_run *r, int t, double d, int inside) {
  r->sum = r->sum + d;
  r->d_last = d;
  r->n += 1;
  r->last = t;
  if (inside) r->cover += 1;
  else if (r->first_out < 0) r->first_out = t;
}
FS_FN double fs_run_ade(const fs_run *r) { return r->n > 0 ? r->sum / (double)r->n : FS_NAN; }
FS_FN double fs_run_fde(const fs_run *r) { return r->n > 0 ? r->d_last : FS_NAN; }

// The sequential pass of one (agent, mode): d[t] and fl[t] (bit 0 = valid, bit 1 = inside) of its T samples; the state is snapshot at each
// horizon into ade / fde / cover / first_out [h * hs]; n_valid / last [h] (the same for every mode of the agent) are written when non-null.
FS_FN void fs_mode_pass(const fs_cfg *c, const double *d, const unsigned char *fl, double *ade, double *fde, int *cover, int *first_out, int hs,
                        int *n_valid, int *last) {
  fs_run r;
  fs_run_init(&r);
  int t = 0;
  for (int h = 0; h < c->n_h; ++h) {
    const int end = c->horizon[h];
    for (; t < end; ++t) {
      const int f = fl[t];
      if (f & 1) fs_run_step(&r, t, d[t], (f >> 1) & 1);
    }
    ade[h * hs] = fs_run_ade(&r);
    fde[h * hs] = fs_run_fde(&r);
    cover[h * hs] = r.cover;
    first_out[h * hs] = r.first_out;
    if (n_valid) n_valid[h] = r.n;
    if (last) last[h] = r.last;
  }
}

// arg-minimum of v[k * stride], k = 0..K-1, as plain C takes it
FS_FN int fs_argmin(const double *v, int K, int stride) {
  double best = FS_INF;
  int kb = -1;
  for (int k = 0; k < K; ++k) {
    const double x = v[k * stride];
    if (x < best) { best = x; kb = k; }
  }
  return kb;
}
// arg-maximum of the mode scores, the lowest k on ties (-1 when every score is NaN or -inf)
FS_FN int fs_argmax_cls(const float *cls, int K) {
  float best = -__builtin_inff();
  int kb = -1;
  for (int k = 0; k < K; ++k) {
    const float x = cls[k];
    if (x > best) { best = x; kb = k; }
  }
  return kb;
}
FS_FN double fs_brier(double fde, float p) {
  const double q = 1.0 - (double)p;
  return fde + q * q;
}

// The (scene, horizon) row over the agents a0 <= a < a1 in index order with scored[a] (NULL = all) and n_valid[a, h] > 0; ade / fde are
// the per-(agent, horizon, mode) arrays [A, n_h, K], n_valid [A, n_h], cls_b the scene's K scores.  s_ade / s_fde point at the row's K values.
FS_FN void fs_scene_pass(const fs_cfg *c, int h, int a0, int a1, const double *ade, const double *fde, const int *n_valid,
                         const unsigned char *scored, const float *cls_b, int *n_scored, double *s_ade, double *s_fde, int *k_ade, int *k_fde,
                         int *k_top, double *brier_fde, double *miss_rate, double *miss_top) {
  const int K = c->K, n_h = c->n_h;
  double sa[FS_MAX_K], sf[FS_MAX_K];
  int ms[FS_MAX_K];
#pragma unroll
  for (int k = 0; k < FS_MAX_K; ++k) { sa[k] = 0.0; sf[k] = 0.0; ms[k] = 0; }
  int n = 0;
  for (int a = a0; a < a1; ++a) {
    if (scored && !scored[a]) continue;
    const size_t row = (size_t)a * (size_t)n_h + (size_t)h;
    if (n_valid[row] <= 0) continue;
    ++n;
#pragma unroll
    for (int k = 0; k < FS_MAX_K; ++k)
      if (k < K) {
        const double f = fde[row * K + k];
        sa[k] = sa[k] + ade[row * K + k];
        sf[k] = sf[k] + f;
        if (f > c->miss_radius) ms[k] += 1;
      }
  }
  double ba = FS_INF, bf = FS_INF, fde_best = FS_NAN;
  float bc = -__builtin_inff(), p_best = 0.f;
  int ka = -1, kf = -1, kt = -1, m_f = 0, m_t = 0;
#pragma unroll
  for (int k = 0; k < FS_MAX_K; ++k)
    if (k < K) {
      const double va = n > 0 ? sa[k] / (double)n : FS_NAN;
      const double vf = n > 0 ? sf[k] / (double)n : FS_NAN;
      s_ade[k] = va;
      s_fde[k] = vf;
      if (va < ba) { ba = va; ka = k; }
      if (vf < bf) { bf = vf; kf = k; fde_best = vf; p_best = cls_b[k]; m_f = ms[k]; }
      if (cls_b[k] > bc) { bc = cls_b[k]; kt = k; m_t = ms[k]; }
    }
  *n_scored = n;
  *k_ade = ka; *k_fde = kf; *k_top = kt;
  *brier_fde = kf >= 0 ? fs_brier(fde_best, p_best) : FS_NAN;
  *miss_rate = (n > 0 && kf >= 0) ? (double)m_f / (double)n : FS_NAN;
  *miss_top = (n > 0 && kt >= 0) ? (double)m_t / (double)n : FS_NAN;
}
