// Forecast scoring on the device: what the predictor said about the other road users against what they went on to do, from forecast_score.h.
//
// k_forecast_modes: per (agent, horizon, mode) ade / fde / cover / first_out, per (agent, horizon) n_valid / last / k_ade / k_fde / brier_fde.
// k_forecast_scenes: per (scene, horizon) the joint rows (one mode index serves every agent of the scene): n_scored, ade[k], fde[k], k_ade,
//   k_fde, brier_fde, miss_rate, k_top, miss_top.
//
// Shapes.  k_forecast_modes: a workgroup of FC_THREADS threads takes nb consecutive agents, nb sized on the host (fc_block) so that the whole
// LDS image of the block fits FC_LDS_BYTES: K = 6, T = 60 gives FC_NB_6_60 agents, K = 8, T = 256 one.  The block's reg rows [nb, K, T, 5], gt
// [nb, T, 2] and valid [nb, T] are one contiguous span each and are staged by all threads with consecutive 16-byte (reg when K T is a
// multiple of 4 and the base is aligned, gt always) or 4-byte / 1-byte loads: no thread walks a 20-byte-strided row of its own in global
// memory.  All threads then compute d and the flag byte (bit 0 valid, bit 1 inside) per sample into LDS rows of Tp doubles / Sb bytes per
// (agent, mode): Tp = 1 (mod 32) puts the rows of consecutive modes two banks apart for the 8-byte reads of the serial pass, Sb = 4 x odd
// one bank apart for its byte reads.  One thread per (agent, mode) runs fs_mode_pass over its row and leaves ade / fde in LDS (the reg
// image is dead by then), one thread per (agent, horizon) takes the arg-minima.  k_forecast_scenes: one thread per (scene, horizon),
// sequential over its agents and modes, as k_audit_plan_trees is.  Every reduction is sequential in one thread: the results do not depend
// on the launch shape; no atomics.
// Included by mind_hip.hip behind audit_kernels.hip.
#pragma clang fp contract(off)
#include "forecast_score.h"

#define FC_THREADS 256
#define FC_LDS_BYTES 65536       // the LDS image of one workgroup of k_forecast_modes (dynamic LDS, no opt-in needed up to 64 KiB)
#define FC_NB_6_60 5             // fc_block(6, 60): agents per workgroup at the predictor's own shape
#define FC_SB 64                 // (scene, horizon) rows per workgroup of k_forecast_scenes

struct FcLay {                   // the LDS image of nb agents: byte offsets, each a multiple of 16
  int Tp, Sb;                    // row lengths of d (doubles) and of the flags (bytes) per (agent, mode)
  unsigned o_reg, o_gt, o_val, o_d, o_fl, bytes;
};
__host__ __device__ constexpr unsigned fc_up16(unsigned v) { return (v + 15u) & ~15u; }
__host__ __device__ constexpr FcLay fc_layout(int K, int T, int nb) {
  FcLay L{};
  L.Tp = ((T - 1 + 31) / 32) * 32 + 1;
  L.Sb = 4 * (((T + 3) / 4) | 1);
  L.o_reg = 0;
  L.o_gt = fc_up16(L.o_reg + (unsigned)nb * K * T * 20u);
  L.o_val = fc_up16(L.o_gt + (unsigned)nb * T * 16u);
  L.o_d = fc_up16(L.o_val + (unsigned)nb * T);
  L.o_fl = fc_up16(L.o_d + (unsigned)nb * K * L.Tp * 8u);
  L.bytes = fc_up16(L.o_fl + (unsigned)nb * K * L.Sb);
  return L;
}
// agents per workgroup: the most whose image fits, at most FC_THREADS / K (one thread per (agent, mode) in the serial pass)
__host__ __device__ constexpr int fc_block(int K, int T) {
  int nb = FC_THREADS / K;
  while (nb > 1 && fc_layout(K, T, nb).bytes > FC_LDS_BYTES) --nb;
  return nb;
}
static_assert(fc_block(6, 60) == FC_NB_6_60, "FC_NB_6_60 is what the tests read");
static_assert(fc_layout(FS_MAX_K, FS_MAX_T, 1).bytes <= FC_LDS_BYTES, "one agent of the largest shape must fit");

__global__ __launch_bounds__(FC_THREADS) void k_forecast_modes(fs_cfg c, int A, int nb, int wide, const float *__restrict__ reg,
                                                               const float *__restrict__ cls, const double *__restrict__ gt,
                                                               const unsigned char *__restrict__ valid, const int *__restrict__ scene_of,
                                                               double *__restrict__ ade, double *__restrict__ fde, int *__restrict__ cover,
                                                               int *__restrict__ first_out, int *__restrict__ n_valid, int *__restrict__ last,
                                                               int *__restrict__ k_ade, int *__restrict__ k_fde, double *__restrict__ brier) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
  const int K = c.K, T = c.T, n_h = c.n_h, KT = K * T;
  const FcLay L = fc_layout(K, T, nb);
  const int tid = threadIdx.x;
  const int a0 = blockIdx.x * nb;
  const int na = A - a0 < nb ? A - a0 : nb;
  float *s_reg = (float *)(fc_lds + L.o_reg);
  double *s_gt = (double *)(fc_lds + L.o_gt);
  unsigned char *s_val = fc_lds + L.o_val;
  double *s_d = (double *)(fc_lds + L.o_d);
  unsigned char *s_fl = fc_lds + L.o_fl;
  {
    // the three spans of the block, consecutive lanes on consecutive addresses
    const float *g_reg = reg + (size_t)a0 * (size_t)KT * 5;
    const int nf = na * KT * 5;
    if (wide) {
      for (int i = tid; i < nf / 4; i += FC_THREADS) ((float4 *)s_reg)[i] = ((const float4 *)g_reg)[i];
    } else {
      for (int i = tid; i < nf; i += FC_THREADS) s_reg[i] = g_reg[i];
    }
    const double2 *g_gt = (const double2 *)(gt + (size_t)a0 * (size_t)T * 2);
    for (int i = tid; i < na * T; i += FC_THREADS) ((double2 *)s_gt)[i] = g_gt[i];
    const unsigned char *g_val = valid + (size_t)a0 * (size_t)T;
    for (int i = tid; i < na * T; i += FC_THREADS) s_val[i] = g_val[i];
  }
  __syncthreads();
  for (int e = tid; e < na * KT; e += FC_THREADS) {
    const int a = e / KT, r = e - a * KT, k = r / T, t = r - k * T;
    int in;
    const double d = fs_sample(s_reg + 5 * e, s_gt[2 * (a * T + t)], s_gt[2 * (a * T + t) + 1], c.disc_scale, c.disc_offset, &in);
    const int row = a * K + k;
    s_d[row * L.Tp + t] = d;
    s_fl[row * L.Sb + t] = (unsigned char)((s_val[a * T + t] != 0 ? 1 : 0) | (in << 1));
  }
  __syncthreads();
  // (the reg image is dead: ade / fde of the block go there in the layout of the outputs, [agent, horizon, mode] each; 16 n_h <= 20 T bytes per
  // (agent, mode))
  double *s_ade = (double *)(fc_lds + L.o_reg), *s_fde = s_ade + (size_t)nb * n_h * K;
  for (int m = tid; m < na * K; m += FC_THREADS) {
    const int a = m / K, k = m - a * K;
    const size_t ah = (size_t)(a0 + a) * (size_t)n_h;
    const int sl = a * n_h * K + k;
    fs_mode_pass(&c, s_d + m * L.Tp, s_fl + m * L.Sb, s_ade + sl, s_fde + sl, cover + ah * K + k, first_out + ah * K + k, K, k == 0 ? n_valid + ah : nullptr,
                 k == 0 ? last + ah : nullptr);
    for (int h = 0; h < n_h; ++h) {
      ade[(ah + h) * K + k] = s_ade[sl + h * K];
      fde[(ah + h) * K + k] = s_fde[sl + h * K];
    }
  }
  __syncthreads();
  for (int j = tid; j < na * n_h; j += FC_THREADS) {
    const int ka = fs_argmin(s_ade + j * K, K, 1), kf = fs_argmin(s_fde + j * K, K, 1);
    const size_t ah = (size_t)a0 * (size_t)n_h + j;
    k_ade[ah] = ka;
    k_fde[ah] = kf;
    brier[ah] = kf >= 0 ? fs_brier(s_fde[j * K + kf], cls[(size_t)scene_of[a0 + j / n_h] * K + kf]) : FS_NAN;
  }
}

__global__ __launch_bounds__(FC_SB) void k_forecast_scenes(fs_cfg c, int n_scenes, const int *__restrict__ actor_off, const float *__restrict__ cls,
                                                           const unsigned char *__restrict__ scored, const double *__restrict__ ade,
                                                           const double *__restrict__ fde, const int *__restrict__ n_valid,
                                                           int *__restrict__ s_n_scored, double *__restrict__ s_ade, double *__restrict__ s_fde,
                                                           int *__restrict__ s_k_ade, int *__restrict__ s_k_fde, int *__restrict__ s_k_top,
                                                           double *__restrict__ s_brier, double *__restrict__ s_miss_rate,
                                                           double *__restrict__ s_miss_top) {
  const long e = (long)blockIdx.x * FC_SB + threadIdx.x;
  if (e >= (long)n_scenes * c.n_h) return;
  const int b = (int)(e / c.n_h), h = (int)(e % c.n_h);
  int n, ka, kf, kt;
  double br, mr, mt;
  fs_scene_pass(&c, h, actor_off[b], actor_off[b + 1], ade, fde, n_valid, scored, cls + (size_t)b * c.K, &n, s_ade + (size_t)e * c.K,
                s_fde + (size_t)e * c.K, &ka, &kf, &kt, &br, &mr, &mt);
  s_n_scored[e] = n; s_k_ade[e] = ka; s_k_fde[e] = kf; s_k_top[e] = kt;
  s_brier[e] = br; s_miss_rate[e] = mr; s_miss_top[e] = mt;
}
