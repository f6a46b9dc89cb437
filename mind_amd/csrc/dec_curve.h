// The decoder's curve step, one text for the two head kernels (k_dec_actor, k_dec_actor_mfma) and the sampling kernel (k_dec_curve): one
// (row, time) of reg / vel / cov_vel from the row's eight control points (x, y, sx, sy, rho) and the basis rows of that time.
//
// Reference: planners/mind/networks/network.py:514-534,545.  pos = T P, cov = exp(T S); vel = Tp diff(P) / 6 under the Bezier basis (:519) and
// Tp P[1:] / 6 under the monomial basis (:530: no diff for positions); cov_vel = Tp diff(S) / 6 under BOTH bases -- the reference applies
// diff to the covariance parameters under the monomial Tp as well (:534), and so does this.
//
// The order of operations is the contract: fmaf over the control points c = 0..7 (0..6), then expf, then / 6.0f.  The heads' reg / vel bits
// are pinned by tests, and k_dec_curve on the heads' own time grid reproduces them because it is this text.
#pragma once

// prm: the row's [8][5] control points (LDS); Tr [8], Tpr [7]: the basis rows of this time; ro [5] / vo [2] / co [3]: the outputs of this
// (row, time), each may be null; monomial: the vel formula (DecW::monomial)
__device__ __forceinline__ void dec_curve_point(const float *prm, const float *__restrict__ Tr, const float *__restrict__ Tpr, int monomial,
                                                float *ro, float *vo, float *co) {
  if (ro) {
    float o5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 8; ++c) {
      const float tv = Tr[c];
#pragma unroll
      for (int d = 0; d < 5; ++d) o5[d] = fmaf(tv, prm[c * 5 + d], o5[d]);
    }
    ro[0] = o5[0]; ro[1] = o5[1]; ro[2] = expf(o5[2]); ro[3] = expf(o5[3]); ro[4] = expf(o5[4]);
  }
  if (vo) {
    float v2[2] = {0.f, 0.f};
    if (monomial) {
      for (int c = 0; c < 7; ++c) {
        const float tv = Tpr[c];
        v2[0] = fmaf(tv, prm[(c + 1) * 5 + 0], v2[0]);
        v2[1] = fmaf(tv, prm[(c + 1) * 5 + 1], v2[1]);
      }
    } else {
      for (int c = 0; c < 7; ++c) {
        const float tv = Tpr[c];
        v2[0] = fmaf(tv, prm[(c + 1) * 5 + 0] - prm[c * 5 + 0], v2[0]);
        v2[1] = fmaf(tv, prm[(c + 1) * 5 + 1] - prm[c * 5 + 1], v2[1]);
      }
    }
    vo[0] = v2[0] / 6.0f; vo[1] = v2[1] / 6.0f;
  }
  if (co) {
    float c3[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < 7; ++c) {
      const float tv = Tpr[c];
#pragma unroll
      for (int d = 0; d < 3; ++d) c3[d] = fmaf(tv, prm[(c + 1) * 5 + 2 + d] - prm[c * 5 + 2 + d], c3[d]);
    }
    co[0] = c3[0] / 6.0f; co[1] = c3[1] / 6.0f; co[2] = c3[2] / 6.0f;
  }
}
