// SceneDecoder's curves at arbitrary times: reg / vel / cov_vel of n_rows rows of eight control points at n_tau times, by the head kernels'
// own contraction (dec_curve.h) over basis rows the host evaluated for those times.  On the decoder's grid the bits are the decoder's.
//
// Reference semantics: planners/mind/networks/network.py:514-534,545 with mat_T / mat_Tp evaluated at tau instead of linspace(0, 1, 60).
//
// One thread per (row, tau), the points numbered p = row * n_tau + t: a workgroup takes DC_T consecutive points, i.e. a contiguous piece of
// each output.  It stages the rows its points fall into once in LDS (40 floats each), every thread writes its 10 results to an LDS image
// of the three pieces, and the pieces go out as consecutive dwords.  10 floats written per point against 15 (cached) table floats and
// 40 / n_tau parameter floats read: a store-bound kernel.  No MFMA.  (Staging the basis rows in LDS as well was measured: the same time at
// 60 samples, 10-25 % slower at 300 -- the table reads are not what bounds it)
#include <hip/hip_runtime.h>

#include "dec_curve.h"

#define DC_T 256
// LDS floats of a launch: the staged rows (a workgroup's DC_T consecutive points touch at most (DC_T - 1) / n_tau + 2 rows) + the output image
static inline int dc_rows_per_block(int n_tau) { return (DC_T - 1) / n_tau + 2; }
static inline size_t dc_lds_bytes(int n_tau) { return ((size_t)dc_rows_per_block(n_tau) * 40 + DC_T * 10) * sizeof(float); }

__global__ __launch_bounds__(DC_T) void k_dec_curve(const float *__restrict__ param /*[n_rows,8,5]*/, int n_pts /* n_rows * n_tau */, int n_tau,
                                                    const float *__restrict__ T /*[n_tau,8]*/, const float *__restrict__ Tp /*[n_tau,7]*/,
                                                    int monomial, float *__restrict__ reg /*[n_rows,n_tau,5]*/,
                                                    float *__restrict__ vel /*[n_rows,n_tau,2]*/, float *__restrict__ cov_vel /*[n_rows,n_tau,3]*/,
                                                    int rows_blk) {
  extern __shared__ __attribute__((aligned(16))) float dcs[];
  float *prm = dcs;                       // [rows_blk][40]
  float *so5 = dcs + rows_blk * 40;       // [DC_T][5], [DC_T][2], [DC_T][3]
  float *so2 = so5 + DC_T * 5;
  float *so3 = so2 + DC_T * 2;
  const int tid = threadIdx.x;
  const int p0 = (int)blockIdx.x * DC_T;
  const int np = min(DC_T, n_pts - p0);
  const int r0 = p0 / n_tau;
  const int nr = (p0 + np - 1) / n_tau - r0 + 1;      // <= rows_blk
  for (int i = tid; i < nr * 40; i += DC_T) prm[i] = param[(size_t)r0 * 40 + i];
  __syncthreads();
  if (tid < np) {
    const int p = p0 + tid;
    const int row = p / n_tau, t = p - row * n_tau;
    dec_curve_point(prm + (row - r0) * 40, T + (size_t)t * 8, Tp + (size_t)t * 7, monomial, reg ? so5 + tid * 5 : nullptr,
                    vel ? so2 + tid * 2 : nullptr, cov_vel ? so3 + tid * 3 : nullptr);
  }
  __syncthreads();
  if (reg)
    for (int i = tid; i < np * 5; i += DC_T) reg[(size_t)p0 * 5 + i] = so5[i];
  if (vel)
    for (int i = tid; i < np * 2; i += DC_T) vel[(size_t)p0 * 2 + i] = so2[i];
  if (cov_vel)
    for (int i = tid; i < np * 3; i += DC_T) cov_vel[(size_t)p0 * 3 + i] = so3[i];
}
