// Host side of the forecast scoring (kernels: forecast_kernels.hip; definitions: forecast_score.h): mind_forecast_score and the host-only
// mind_debug_forecast_score.  The device call is synchronous on the context's stream and keeps its scratch in c->forecast_dev.
// Included by mind_hip.hip behind audit_host.hip.
#pragma clang fp contract(off)

#define FC_MAX_AGENTS (1L << 20)

// every MIND_EINVAL of the two entries; fills the kernels' configuration and the agent count.  `msg` receives what was wrong.
static int fc_check(const mind_forecast_cfg *cfg, int n_scenes, const int32_t *actor_off, const void *reg, const void *cls, const double *gt,
                    const uint8_t *valid, const mind_forecast_out *out, fs_cfg *fc, long *A_out, char *msg, size_t n_msg) {
#define FC_BAD(...) do { snprintf(msg, n_msg, __VA_ARGS__); return MIND_EINVAL; } while (0)
  if (!cfg || !out || !cfg->horizon) FC_BAD("null cfg / cfg->horizon / out");
  if (cfg->K < 1 || cfg->K > FS_MAX_K || cfg->T < 1 || cfg->T > FS_MAX_T || cfg->n_h < 1 || cfg->n_h > FS_MAX_H)
    FC_BAD("K = %d, T = %d, n_h = %d: 1..%d modes, 1..%d samples and 1..%d horizons are supported", cfg->K, cfg->T, cfg->n_h, FS_MAX_K, FS_MAX_T, FS_MAX_H);
  for (int h = 0; h < cfg->n_h; ++h)
    if (cfg->horizon[h] < 1 || cfg->horizon[h] > cfg->T || (h > 0 && cfg->horizon[h] <= cfg->horizon[h - 1]))
      FC_BAD("horizon[%d] = %d: the horizons must ascend strictly within 1..T = %d", h, cfg->horizon[h], cfg->T);
  const double par[3] = {cfg->miss_radius, cfg->disc_scale, cfg->disc_offset};
  for (double v : par)
    if (!std::isfinite(v) || v < 0.0) FC_BAD("miss_radius = %g, disc_scale = %g, disc_offset = %g: finite values >= 0 are needed", par[0], par[1], par[2]);
  if (!out->ade && !out->fde && !out->cover && !out->first_out && !out->n_valid && !out->last && !out->k_ade && !out->k_fde && !out->brier_fde &&
      !out->s_n_scored && !out->s_ade && !out->s_fde && !out->s_k_ade && !out->s_k_fde && !out->s_k_top && !out->s_brier_fde && !out->s_miss_rate &&
      !out->s_miss_top)
    FC_BAD("every output is null");
  if (n_scenes < 0 || (n_scenes > 0 && !actor_off)) FC_BAD("a negative scene count or null actor_off");
  long A = 0;
  if (n_scenes > 0) {
    if (actor_off[0] != 0) FC_BAD("actor_off[0] = %d, 0 is needed", actor_off[0]);
    for (int b = 0; b < n_scenes; ++b)
      if (actor_off[b + 1] < actor_off[b]) FC_BAD("actor_off[%d] = %d < actor_off[%d] = %d", b + 1, actor_off[b + 1], b, actor_off[b]);
    A = actor_off[n_scenes];
  }
  if (A > FC_MAX_AGENTS) FC_BAD("%ld agents > %ld supported", A, FC_MAX_AGENTS);
  if (A > 0 && (!reg || !cls || !gt || !valid)) FC_BAD("null reg / cls / gt / valid");
  const size_t T = cfg->T;
  for (size_t i = 0; i < (size_t)A * T; ++i)
    if (valid[i] && (!std::isfinite(gt[i * 2]) || !std::isfinite(gt[i * 2 + 1])))
      FC_BAD("agent %ld sample %ld: valid but gt is not finite", (long)(i / T), (long)(i % T));
#undef FC_BAD
  fc->K = cfg->K; fc->T = cfg->T; fc->n_h = cfg->n_h;
  for (int h = 0; h < FS_MAX_H; ++h) fc->horizon[h] = h < cfg->n_h ? cfg->horizon[h] : 0;
  fc->miss_radius = cfg->miss_radius; fc->disc_scale = cfg->disc_scale; fc->disc_offset = cfg->disc_offset;
  *A_out = A;
  return MIND_OK;
}

extern "C" int mind_forecast_score(mind_ctx *c, const mind_forecast_cfg *cfg, int n_scenes, const int32_t *actor_off, const float *reg, const float *cls,
                                   const double *gt, const uint8_t *valid, const uint8_t *scored, const mind_forecast_out *out) {
  const char *who = "mind_forecast_score";
  if (!c) return MIND_EINVAL;
  fs_cfg fc;
  long Al = 0;
  char msg[256];
  if (fc_check(cfg, n_scenes, actor_off, reg, cls, gt, valid, out, &fc, &Al, msg, sizeof msg)) return fail(c, MIND_EINVAL, "%s: %s", who, msg);
  int rc;
  if ((rc = au_busy(c, who))) return rc;
  if (Al == 0 || n_scenes == 0) return MIND_OK;

  const size_t A = (size_t)Al, B = (size_t)n_scenes, K = fc.K, T = fc.T, H = fc.n_h;
  std::vector<int32_t> scene_of(A);
  for (size_t b = 0; b < B; ++b)
    for (int32_t a = actor_off[b]; a < actor_off[b + 1]; ++a) scene_of[a] = (int32_t)b;
  // the arena: inputs (gt, valid, scored, scene_of, actor_off), then outputs
  size_t top = 0;
  const size_t o_gt = au_take(top, A * T * 2, sizeof(double)), o_val = au_take(top, A * T, 1), o_sc = au_take(top, A, 1), o_so = au_take(top, A, sizeof(int)),
               o_off = au_take(top, B + 1, sizeof(int));
  const size_t o_ade = au_take(top, A * H * K, sizeof(double)), o_fde = au_take(top, A * H * K, sizeof(double)), o_cov = au_take(top, A * H * K, sizeof(int)),
               o_fo = au_take(top, A * H * K, sizeof(int)), o_nv = au_take(top, A * H, sizeof(int)), o_last = au_take(top, A * H, sizeof(int)),
               o_ka = au_take(top, A * H, sizeof(int)), o_kf = au_take(top, A * H, sizeof(int)), o_br = au_take(top, A * H, sizeof(double));
  const size_t o_sn = au_take(top, B * H, sizeof(int)), o_sa = au_take(top, B * H * K, sizeof(double)), o_sf = au_take(top, B * H * K, sizeof(double)),
               o_ska = au_take(top, B * H, sizeof(int)), o_skf = au_take(top, B * H, sizeof(int)), o_skt = au_take(top, B * H, sizeof(int)),
               o_sbr = au_take(top, B * H, sizeof(double)), o_smr = au_take(top, B * H, sizeof(double)), o_smt = au_take(top, B * H, sizeof(double));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->forecast_dev, top))) return rc;
  char *d = (char *)c->forecast_dev.p;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d + o_gt, gt, A * T * 2 * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d + o_val, valid, A * T, hipMemcpyHostToDevice, s));
  if (scored) HIPCHK(c, hipMemcpyAsync(d + o_sc, scored, A, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d + o_so, scene_of.data(), A * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d + o_off, actor_off, (B + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  const int nb = fc_block(fc.K, fc.T);
  const FcLay L = fc_layout(fc.K, fc.T, nb);
  const int wide = (K * T) % 4 == 0 && ((uintptr_t)reg % 16) == 0;
  hipLaunchKernelGGL(k_forecast_modes, dim3((unsigned)((A + nb - 1) / nb)), dim3(FC_THREADS), L.bytes, s, fc, (int)A, nb, wide, reg, cls, (const double *)(d + o_gt),
                     (const unsigned char *)(d + o_val), (const int *)(d + o_so), (double *)(d + o_ade), (double *)(d + o_fde), (int *)(d + o_cov),
                     (int *)(d + o_fo), (int *)(d + o_nv), (int *)(d + o_last), (int *)(d + o_ka), (int *)(d + o_kf), (double *)(d + o_br));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_forecast_scenes, dim3((unsigned)((B * H + FC_SB - 1) / FC_SB)), dim3(FC_SB), 0, s, fc, n_scenes, (const int *)(d + o_off), cls,
                     scored ? (const unsigned char *)(d + o_sc) : (const unsigned char *)nullptr, (const double *)(d + o_ade), (const double *)(d + o_fde),
                     (const int *)(d + o_nv), (int *)(d + o_sn), (double *)(d + o_sa), (double *)(d + o_sf), (int *)(d + o_ska), (int *)(d + o_skf),
                     (int *)(d + o_skt), (double *)(d + o_sbr), (double *)(d + o_smr), (double *)(d + o_smt));
  HIPCHK(c, hipGetLastError());
  const struct { void *h; size_t o, bytes; } back[18] = {
      {out->ade, o_ade, A * H * K * sizeof(double)},   {out->fde, o_fde, A * H * K * sizeof(double)},   {out->cover, o_cov, A * H * K * sizeof(int)},
      {out->first_out, o_fo, A * H * K * sizeof(int)}, {out->n_valid, o_nv, A * H * sizeof(int)},       {out->last, o_last, A * H * sizeof(int)},
      {out->k_ade, o_ka, A * H * sizeof(int)},         {out->k_fde, o_kf, A * H * sizeof(int)},         {out->brier_fde, o_br, A * H * sizeof(double)},
      {out->s_n_scored, o_sn, B * H * sizeof(int)},    {out->s_ade, o_sa, B * H * K * sizeof(double)},  {out->s_fde, o_sf, B * H * K * sizeof(double)},
      {out->s_k_ade, o_ska, B * H * sizeof(int)},      {out->s_k_fde, o_skf, B * H * sizeof(int)},      {out->s_k_top, o_skt, B * H * sizeof(int)},
      {out->s_brier_fde, o_sbr, B * H * sizeof(double)}, {out->s_miss_rate, o_smr, B * H * sizeof(double)}, {out->s_miss_top, o_smt, B * H * sizeof(double)}};
  for (const auto &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.o, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MIND_OK;
}

// forecast_score.h on the CPU: the same passes, agent after agent
extern "C" int mind_debug_forecast_score(const mind_forecast_cfg *cfg, int n_scenes, const int32_t *actor_off, const float *reg, const float *cls,
                                         const double *gt, const uint8_t *valid, const uint8_t *scored, const mind_forecast_out *out) {
  fs_cfg fc;
  long Al = 0;
  char msg[256];
  if (fc_check(cfg, n_scenes, actor_off, reg, cls, gt, valid, out, &fc, &Al, msg, sizeof msg)) return MIND_EINVAL;
  if (Al == 0 || n_scenes == 0) return MIND_OK;
  const size_t A = (size_t)Al, B = (size_t)n_scenes, K = fc.K, T = fc.T, H = fc.n_h;
  std::vector<double> ade(A * H * K), fde(A * H * K), brier(A * H), s_ade(B * H * K), s_fde(B * H * K), s_br(B * H), s_mr(B * H), s_mt(B * H);
  std::vector<int32_t> cover(A * H * K), first_out(A * H * K), n_valid(A * H), last(A * H), k_ade(A * H), k_fde(A * H), s_n(B * H), s_ka(B * H), s_kf(B * H),
      s_kt(B * H);
  std::vector<double> dd(K * T);
  std::vector<unsigned char> fl(K * T);
  size_t b = 0;
  for (size_t a = 0; a < A; ++a) {
    while ((size_t)actor_off[b + 1] <= a) ++b;
    for (size_t k = 0; k < K; ++k)
      for (size_t t = 0; t < T; ++t) {
        int in;
        dd[k * T + t] = fs_sample(reg + ((a * K + k) * T + t) * 5, gt[(a * T + t) * 2], gt[(a * T + t) * 2 + 1], fc.disc_scale, fc.disc_offset, &in);
        fl[k * T + t] = (unsigned char)((valid[a * T + t] != 0 ? 1 : 0) | (in << 1));
      }
    const size_t ah = a * H;
    for (size_t k = 0; k < K; ++k)
      fs_mode_pass(&fc, dd.data() + k * T, fl.data() + k * T, ade.data() + ah * K + k, fde.data() + ah * K + k, cover.data() + ah * K + k,
                   first_out.data() + ah * K + k, (int)K, k == 0 ? n_valid.data() + ah : nullptr, k == 0 ? last.data() + ah : nullptr);
    for (size_t h = 0; h < H; ++h) {
      const int ka = fs_argmin(ade.data() + (ah + h) * K, (int)K, 1), kf = fs_argmin(fde.data() + (ah + h) * K, (int)K, 1);
      k_ade[ah + h] = ka;
      k_fde[ah + h] = kf;
      brier[ah + h] = kf >= 0 ? fs_brier(fde[(ah + h) * K + kf], cls[b * K + kf]) : FS_NAN;
    }
  }
  for (size_t e = 0; e < B * H; ++e) {
    const size_t sb = e / H;
    fs_scene_pass(&fc, (int)(e % H), actor_off[sb], actor_off[sb + 1], ade.data(), fde.data(), n_valid.data(), scored, cls + sb * K, &s_n[e], s_ade.data() + e * K,
                  s_fde.data() + e * K, &s_ka[e], &s_kf[e], &s_kt[e], &s_br[e], &s_mr[e], &s_mt[e]);
  }
  const struct { void *h; const void *src; size_t bytes; } back[18] = {
      {out->ade, ade.data(), A * H * K * sizeof(double)},      {out->fde, fde.data(), A * H * K * sizeof(double)},
      {out->cover, cover.data(), A * H * K * sizeof(int)},     {out->first_out, first_out.data(), A * H * K * sizeof(int)},
      {out->n_valid, n_valid.data(), A * H * sizeof(int)},     {out->last, last.data(), A * H * sizeof(int)},
      {out->k_ade, k_ade.data(), A * H * sizeof(int)},         {out->k_fde, k_fde.data(), A * H * sizeof(int)},
      {out->brier_fde, brier.data(), A * H * sizeof(double)},  {out->s_n_scored, s_n.data(), B * H * sizeof(int)},
      {out->s_ade, s_ade.data(), B * H * K * sizeof(double)},  {out->s_fde, s_fde.data(), B * H * K * sizeof(double)},
      {out->s_k_ade, s_ka.data(), B * H * sizeof(int)},        {out->s_k_fde, s_kf.data(), B * H * sizeof(int)},
      {out->s_k_top, s_kt.data(), B * H * sizeof(int)},        {out->s_brier_fde, s_br.data(), B * H * sizeof(double)},
      {out->s_miss_rate, s_mr.data(), B * H * sizeof(double)}, {out->s_miss_top, s_mt.data(), B * H * sizeof(double)}};
  for (const auto &r : back)
    if (r.h) memcpy(r.h, r.src, r.bytes);
  return MIND_OK;
}
