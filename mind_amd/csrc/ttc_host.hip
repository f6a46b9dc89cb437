// Host side of the time-to-collision audit (kernel: ttc_kernels.hip; geometry: ttc_geom.h): mind_audit_ttc and the host-only
// mind_debug_box_ttc.  The device call is synchronous on the context's stream and runs on the scaffold of audit_host.hip.
// Included by mind_hip.hip behind road_host.hip (au_host::mind_sincos, au_fin, au_box_ok, au_busy, ar_*, the row caps: audit_host.hip).
#pragma clang fp contract(off)

// The lane layout of k_audit_ttc when the caller leaves it to the library (cfg.lanes == 0) -- the ONE place that decides it.
// Thread per ego (1) launches n_steps x ceil(n_ego / 64) wavefronts whose lanes each walk all n_tracks - 1 tracks one after the other: its
// time is the latency of that walk (0.9 us per track) for as long as those wavefronts leave the device empty.  Lanes over tracks (2)
// launches n_ego x n_steps wavefronts that each stage the step's tracks once more (a sin / cos per track) and evaluate one pair per lane
// and 64-track turn: no walk, but work that grows with every (ego, step) row.  Measured on the 40-track demo_1 scene (DESIGN 5g,
// profiles/ttc_kernel_times.txt): (1) takes 36 us from 1 to 64 egos x 546 steps and 106 us at 4 096 x 100; (2) takes 6.6 us + 1.0 ns per
// row -- 22.7 us at 32 x 546 = 17 472 rows, 40.6 us at 64 x 546 = 34 944, 402 us at 409 600.  They cross at about 30 000 rows, whatever
// n_ego and n_steps multiply to it, so the rule is in rows.  A scene of far more tracks moves the crossing up ((1)'s walk grows by the
// track, (2)'s work by the turn of 64); none has been measured, and the rule errs towards (1) there by at most the walk.
#define TT_LANES2_MAX_ROWS (1L << 15)     // (2) up to here, (1) above
static int tt_lanes(int n_ego, int n_steps) { return (long)n_ego * (long)n_steps <= TT_LANES2_MAX_ROWS ? 2 : 1; }

extern "C" int mind_audit_ttc(mind_ctx *c, const mind_audit_box *ego, const mind_audit_ttc_cfg *cfg, int n_ego, int n_steps, int n_tracks,
                              const double *ego_states, const double *exo, const uint8_t *valid, const double *boxes, const mind_audit_ttc_out *out) {
  const char *who = "mind_audit_ttc";
  if (!c) return MIND_EINVAL;
  if (!ego || !cfg || !out || n_ego < 0 || n_steps < 0 || n_tracks < 1) return fail(c, MIND_EINVAL, "%s: null ego / cfg / out, a negative count or no track row", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  if (!au_fin(cfg->horizon) || !(cfg->horizon > 0.0)) return fail(c, MIND_EINVAL, "%s: horizon = %g, a finite value > 0 is needed", who, cfg->horizon);
  if (!au_fin(cfg->bound) || cfg->bound < 0.0) return fail(c, MIND_EINVAL, "%s: bound = %g, a finite value >= 0 is needed", who, cfg->bound);
  if (cfg->lanes < 0 || cfg->lanes > 2) return fail(c, MIND_EINVAL, "%s: lanes = %d; 0 (the library's rule), 1 (thread per ego) or 2 (lanes over tracks)", who, cfg->lanes);
  if (!out->step_ttc && !out->step_track && !out->ego_min && !out->ego_step && !out->ego_track && !out->ego_hits && !out->ego_first)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  const size_t R = (size_t)n_ego * (size_t)n_steps, RS = (size_t)n_steps * (size_t)n_tracks;
  if ((long)R > AU_EPISODE_MAX_ROWS || n_ego > 65535 * AU_EB) return fail(c, MIND_EINVAL, "%s: %d egos x %d steps > %ld rows supported", who, n_ego, n_steps, AU_EPISODE_MAX_ROWS);
  if ((long)RS > AU_SCENE_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d steps x %d tracks > %ld rows supported", who, n_steps, n_tracks, AU_SCENE_MAX_ROWS);
  if (R > 0 && (!ego_states || (n_tracks > 1 && (!exo || !valid || !boxes)))) return fail(c, MIND_EINVAL, "%s: null ego_states / exo / valid / boxes", who);
  if (R > 0) {
    for (int j = 1; j < n_tracks; ++j)
      if (!au_fin(boxes[j * 2]) || !au_fin(boxes[j * 2 + 1]) || boxes[j * 2] < 0.0 || boxes[j * 2 + 1] < 0.0)
        return fail(c, MIND_EINVAL, "%s: track %d: non-finite or negative box dimension", who, j);
    for (size_t i = 0; i < R * 4; ++i)
      if (!au_fin(ego_states[i])) return fail(c, MIND_EINVAL, "%s: ego %ld step %ld: non-finite state", who, (long)(i / 4 / n_steps), (long)(i / 4 % n_steps));
    for (size_t i = 0; i < RS; ++i)
      if (i % n_tracks != 0 && valid[i])
        for (int q = 0; q < 5; ++q)
          if (!au_fin(exo[i * 5 + q])) return fail(c, MIND_EINVAL, "%s: step %ld track %ld: valid but not finite", who, (long)(i / n_tracks), (long)(i % n_tracks));
  }
  int rc;
  if ((rc = au_busy(c, who))) return rc;
  if (R == 0) return MIND_OK;

  const size_t ne = (size_t)n_ego;
  Arena ar;
  const auto f_ego = ar.take<double>(R * 4), f_exo = ar.take<double>(RS * 5), f_box = ar.take<double>((size_t)n_tracks * 2);
  const auto f_val = ar.take<uint8_t>(RS);
  const auto f_ttc = ar.take<double>(R);
  const auto f_track = ar.take<int>(R);
  const auto f_emin = ar.take<double>(ne);
  const auto f_estep = ar.take<int>(ne), f_etrack = ar.take<int>(ne), f_ehits = ar.take<int>(ne), f_efirst = ar.take<int>(ne);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ar_put(c, d, f_ego, ego_states))) return rc;
  // without a track beside the ego's row the scene is not uploaded: k_audit_ttc's loop over the tracks 1..n-1 reads none of it
  if (n_tracks > 1 && ((rc = ar_put(c, d, f_exo, exo)) || (rc = ar_put(c, d, f_box, boxes)) || (rc = ar_put(c, d, f_val, valid)))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  const int lanes = cfg->lanes ? cfg->lanes : tt_lanes(n_ego, n_steps);
  // one workgroup per (step, block of 64 egos) or per (step, ego): at most 2^22 either way
  if (lanes == 1)
    hipLaunchKernelGGL(k_audit_ttc<1>, dim3((unsigned)((size_t)n_steps * (size_t)((n_ego + AU_EB - 1) / AU_EB))), dim3(AU_EB), 0, s, eb, cfg->horizon, n_ego, n_steps,
                       n_tracks, f_ego.at(d), f_exo.at(d), f_val.at(d), f_box.at(d), f_ttc.at(d), f_track.at(d));
  else
    hipLaunchKernelGGL(k_audit_ttc<2>, dim3((unsigned)R), dim3(AU_EB), 0, s, eb, cfg->horizon, n_ego, n_steps, n_tracks, f_ego.at(d), f_exo.at(d), f_val.at(d),
                       f_box.at(d), f_ttc.at(d), f_track.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_episode_egos<false>, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, cfg->bound, f_ttc.at(d), f_track.at(d),
                     f_emin.at(d), f_estep.at(d), f_etrack.at(d), f_ehits.at(d), f_efirst.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->step_ttc, f_ttc}, {out->step_track, f_track}, {out->ego_min, f_emin}, {out->ego_step, f_estep},
                          {out->ego_track, f_etrack}, {out->ego_hits, f_ehits}, {out->ego_first, f_efirst}});
}

extern "C" int mind_debug_box_ttc(int n, const double *a, const double *b, const double *trig, double *out) {
  if (n < 0 || (n > 0 && (!a || !b || !out))) return MIND_EINVAL;
  for (int i = 0; i < n; ++i) {
    const double *A = a + (size_t)i * 7, *B = b + (size_t)i * 7;
    double ca, sa, cb, sb;
    if (trig) {
      ca = trig[(size_t)i * 4]; sa = trig[(size_t)i * 4 + 1]; cb = trig[(size_t)i * 4 + 2]; sb = trig[(size_t)i * 4 + 3];
    } else {
      au_host::mind_sincos(A[2], &sa, &ca);
      au_host::mind_sincos(B[2], &sb, &cb);
    }
    out[i] = tg_rect_rect_ttc(B[0] - A[0], B[1] - A[1], B[5] - A[5], B[6] - A[6], ca, sa, A[3], A[4], cb, sb, B[3], B[4]);
  }
  return MIND_OK;
}
