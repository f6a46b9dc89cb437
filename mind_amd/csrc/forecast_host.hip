// Host side of the forecast scoring (kernels: forecast_kernels.hip; definitions: forecast_score.h): mind_forecast_score and the host-only
// mind_debug_forecast_score.  The device call is synchronous on the context's stream and runs on the scaffold of audit_host.hip.
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
  // the arena: inputs (gt, valid, scored, scene_of, actor_off), then outputs.  Without `scored` its field is not uploaded, and
  // k_forecast_scenes gets a null pointer for it: nothing reads what an earlier call left there
  Arena ar;
  const auto f_gt = ar.take<double>(A * T * 2);
  const auto f_val = ar.take<uint8_t>(A * T), f_sc = ar.take<uint8_t>(A);
  const auto f_so = ar.take<int>(A), f_off = ar.take<int>(B + 1);
  const auto f_ade = ar.take<double>(A * H * K), f_fde = ar.take<double>(A * H * K);
  const auto f_cov = ar.take<int>(A * H * K), f_fo = ar.take<int>(A * H * K), f_nv = ar.take<int>(A * H), f_last = ar.take<int>(A * H),
             f_ka = ar.take<int>(A * H), f_kf = ar.take<int>(A * H);
  const auto f_br = ar.take<double>(A * H);
  const auto f_sn = ar.take<int>(B * H);
  const auto f_sa = ar.take<double>(B * H * K), f_sf = ar.take<double>(B * H * K);
  const auto f_ska = ar.take<int>(B * H), f_skf = ar.take<int>(B * H), f_skt = ar.take<int>(B * H);
  const auto f_sbr = ar.take<double>(B * H), f_smr = ar.take<double>(B * H), f_smt = ar.take<double>(B * H);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ar_put(c, d, f_gt, gt)) || (rc = ar_put(c, d, f_val, valid)) || (scored && (rc = ar_put(c, d, f_sc, scored))) ||
      (rc = ar_put(c, d, f_so, scene_of.data())) || (rc = ar_put(c, d, f_off, actor_off)))
    return rc;
  const int nb = fc_block(fc.K, fc.T);
  const FcLay L = fc_layout(fc.K, fc.T, nb);
  const int wide = (K * T) % 4 == 0 && ((uintptr_t)reg % 16) == 0;
  hipLaunchKernelGGL(k_forecast_modes, dim3((unsigned)((A + nb - 1) / nb)), dim3(FC_THREADS), L.bytes, s, fc, (int)A, nb, wide, reg, cls, f_gt.at(d), f_val.at(d),
                     f_so.at(d), f_ade.at(d), f_fde.at(d), f_cov.at(d), f_fo.at(d), f_nv.at(d), f_last.at(d), f_ka.at(d), f_kf.at(d), f_br.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_forecast_scenes, dim3((unsigned)((B * H + FC_SB - 1) / FC_SB)), dim3(FC_SB), 0, s, fc, n_scenes, f_off.at(d), cls,
                     scored ? f_sc.at(d) : nullptr, f_ade.at(d), f_fde.at(d), f_nv.at(d), f_sn.at(d), f_sa.at(d), f_sf.at(d), f_ska.at(d), f_skf.at(d),
                     f_skt.at(d), f_sbr.at(d), f_smr.at(d), f_smt.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->ade, f_ade}, {out->fde, f_fde}, {out->cover, f_cov}, {out->first_out, f_fo}, {out->n_valid, f_nv}, {out->last, f_last},
                          {out->k_ade, f_ka}, {out->k_fde, f_kf}, {out->brier_fde, f_br}, {out->s_n_scored, f_sn}, {out->s_ade, f_sa}, {out->s_fde, f_sf},
                          {out->s_k_ade, f_ska}, {out->s_k_fde, f_skf}, {out->s_k_top, f_skt}, {out->s_brier_fde, f_sbr}, {out->s_miss_rate, f_smr},
                          {out->s_miss_top, f_smt}});
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
  const auto give = [](auto *h, const auto &v) { if (h) std::copy(v.begin(), v.end(), h); };      // (every output is optional)
  give(out->ade, ade); give(out->fde, fde); give(out->cover, cover); give(out->first_out, first_out); give(out->n_valid, n_valid); give(out->last, last);
  give(out->k_ade, k_ade); give(out->k_fde, k_fde); give(out->brier_fde, brier); give(out->s_n_scored, s_n); give(out->s_ade, s_ade); give(out->s_fde, s_fde);
  give(out->s_k_ade, s_ka); give(out->s_k_fde, s_kf); give(out->s_k_top, s_kt); give(out->s_brier_fde, s_br); give(out->s_miss_rate, s_mr);
  give(out->s_miss_top, s_mt);
  return MIND_OK;
}
