// What mind_weights_load decides without a device: the reference state_dict re-laid into the packed blob (wp_pack: one function per network
// over the packers below -- transposes, MFMA fragment orders, bf16 splits, folded LayerNorm centring) and the blob bound to the kernels' pointer
// tables (wp_bind, weight_tables.h).  The two halves meet only in the blob's string keys, so the binder checks them: a key the packer did not
// add fails the bind by name instead of handing a kernel a null pointer.  Standard library only, no HIP call, no context: tests read the packers,
// the image and the binder through mind_debug_pack / mind_debug_weight_image / mind_debug_weight_bind.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "weight_tables.h"

struct WeightBlob {
  struct Entry { std::string key; size_t off, len; };
  std::vector<float> host;
  std::map<std::string, size_t> off;
  std::vector<Entry> entries;       // in the order they were added
  size_t add(const std::string &key, const std::vector<float> &v) {
    while (host.size() % 64) host.push_back(0.f);  // 256-byte alignment
    size_t o = host.size();
    host.insert(host.end(), v.begin(), v.end());
    off[key] = o;
    entries.push_back({key, o, v.size()});
    return o;
  }
};

struct SD {
  std::map<std::string, std::pair<const float *, int64_t>> m;
  std::string missing;
  const float *get(const std::string &k, int64_t numel) {
    auto it = m.find(k);
    if (it == m.end() || it->second.second != numel) {
      if (missing.empty()) missing = k;
      return nullptr;
    }
    return it->second.first;
  }
};

// -------------------------------------------------------------------------------------------------
// packers
// -------------------------------------------------------------------------------------------------
inline std::vector<float> vec(const float *p, size_t n) { return p ? std::vector<float>(p, p + n) : std::vector<float>(n, 0.f); }

// [out][in] -> [in][out]
inline std::vector<float> transpose(const float *w, int n_out, int n_in, int row_stride = -1, int col0 = 0) {
  if (row_stride < 0) row_stride = n_in;
  std::vector<float> t((size_t)n_out * n_in, 0.f);
  if (!w) return t;
  for (int o = 0; o < n_out; ++o)
    for (int k = 0; k < n_in; ++k) t[(size_t)k * n_out + o] = w[(size_t)o * row_stride + col0 + k];
  return t;
}

// MFMA 16x16x4 A-fragment order: [ob 8][s4 8][lane 64][w 4] = W[16 ob + (lane&15)][16 s4 + 4 (lane>>4) + w]
inline std::vector<float> pack_afrag(const float *w, int row_stride) {
  std::vector<float> t(16384, 0.f);
  if (!w) return t;
  for (int ob = 0; ob < 8; ++ob)
    for (int s4 = 0; s4 < 8; ++s4)
      for (int lane = 0; lane < 64; ++lane)
        for (int k = 0; k < 4; ++k)
          t[((size_t)(ob * 8 + s4) * 64 + lane) * 4 + k] =
              w[(size_t)(16 * ob + (lane & 15)) * row_stride + 16 * s4 + 4 * (lane >> 4) + k];
  return t;
}

// folded-K-query fragments of k_token_mfma: per head hd and output block ob the A operand [16 features] x [16 d]:
// [hd 8][ob 8][lane 64][w 4] = Wk[hd * 16 + 4 (lane >> 4) + w][16 ob + (lane & 15)]   (Wk = rows 128..255 of in_proj_weight)
inline std::vector<float> pack_wk_frag(const float *wk) {
  std::vector<float> t(16384, 0.f);
  if (!wk) return t;
  for (int hd = 0; hd < 8; ++hd)
    for (int ob = 0; ob < 8; ++ob)
      for (int lane = 0; lane < 64; ++lane)
        for (int k = 0; k < 4; ++k)
          t[((size_t)(hd * 8 + ob) * 64 + lane) * 4 + k] = wk[(size_t)(hd * 16 + 4 * (lane >> 4) + k) * 128 + 16 * ob + (lane & 15)];
  return t;
}

// round-to-nearest-even bf16 of a float (bits), and the split x = hi + lo
inline uint16_t bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// bf16 MFMA 16x16x32 A-fragment order, hi and lo parts: [part 2][ob 8][g 4][lane 64][dword 4]; dword d of lane
// (r = lane & 15, q = lane >> 4) packs k-slots 2d, 2d+1; k-slot (q, i) <-> input feature 16 (2g + (i >> 2)) + 4q + (i & 3)
// (the chained B-operand order of pair_bf16_kernels.hip).  Returned as float bit patterns (16384 dwords).
// the third part of the exact three-way split x = hi + mid + lo (mid = pack_bfrag's lo part), same fragment order: [ob 8][g 4][lane 64][dword 4]
inline std::vector<float> pack_bfrag_lo3(const std::vector<float> &w, int row_stride) {
  std::vector<uint32_t> t(8192, 0u);
  for (int ob = 0; ob < 8; ++ob)
    for (int g = 0; g < 4; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int d = 0; d < 4; ++d) {
          uint32_t lo = 0;
          for (int e = 0; e < 2; ++e) {
            const int i = 2 * d + e, q = lane >> 4;
            const int f = 16 * (2 * g + (i >> 2)) + 4 * q + (i & 3);
            const float x = w[(size_t)(16 * ob + (lane & 15)) * row_stride + f];
            const float r1 = x - bf16_to_f32(bf16_rne(x));
            const float r2 = r1 - bf16_to_f32(bf16_rne(r1));
            lo |= (uint32_t)bf16_rne(r2) << (16 * e);
          }
          t[((size_t)(ob * 4 + g) * 64 + lane) * 4 + d] = lo;
        }
  std::vector<float> out(8192);
  memcpy(out.data(), t.data(), 8192 * sizeof(float));
  return out;
}

inline std::vector<float> pack_bfrag(const std::vector<float> &w, int row_stride) {
  std::vector<uint32_t> t(16384, 0u);
  for (int ob = 0; ob < 8; ++ob)
    for (int g = 0; g < 4; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int d = 0; d < 4; ++d) {
          uint32_t hi = 0, lo = 0;
          for (int e = 0; e < 2; ++e) {
            const int i = 2 * d + e, q = lane >> 4;
            const int f = 16 * (2 * g + (i >> 2)) + 4 * q + (i & 3);
            const float x = w[(size_t)(16 * ob + (lane & 15)) * row_stride + f];
            const uint16_t h = bf16_rne(x);
            const uint16_t l = bf16_rne(x - bf16_to_f32(h));
            hi |= (uint32_t)h << (16 * e);
            lo |= (uint32_t)l << (16 * e);
          }
          const size_t o = ((size_t)(ob * 4 + g) * 64 + lane) * 4 + d;
          t[o] = hi;
          t[8192 + o] = lo;
        }
  std::vector<float> out(16384);
  memcpy(out.data(), t.data(), 16384 * sizeof(float));
  return out;
}

// k_token_mfma<1> (bf16 hi + lo split operands): A fragments of a [128 out] x [128 in] block of w (row stride row_stride) for the bf16 MFMA
// 16x16x32 in NATURAL k order -- the B operand is read from an fp32 LDS tile, 8 consecutive features per lane --:
// [ob 8][s 8 = part * 4 + g][lane 64][dword 4]; dword d of lane (r = lane & 15, q = lane >> 4) packs W[16 ob + r][32 g + 8 q + 2 d (+ 1)].
// Same addressing as pack_afrag's (tm_load reads both), returned as float bit patterns (16384 dwords).
inline std::vector<float> pack_tok_bfrag(const float *w, int row_stride) {
  std::vector<uint32_t> t(16384, 0u);
  if (w)
    for (int ob = 0; ob < 8; ++ob)
      for (int g = 0; g < 4; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int d = 0; d < 4; ++d) {
            uint32_t hi = 0, lo = 0;
            for (int e = 0; e < 2; ++e) {
              const float x = w[(size_t)(16 * ob + (lane & 15)) * row_stride + 32 * g + 8 * (lane >> 4) + 2 * d + e];
              const uint16_t h = bf16_rne(x);
              const uint16_t l = bf16_rne(x - bf16_to_f32(h));
              hi |= (uint32_t)h << (16 * e);
              lo |= (uint32_t)l << (16 * e);
            }
            t[((size_t)(ob * 8 + g) * 64 + lane) * 4 + d] = hi;
            t[((size_t)(ob * 8 + 4 + g) * 64 + lane) * 4 + d] = lo;
          }
  std::vector<float> f(16384);
  memcpy(f.data(), t.data(), 16384 * sizeof(float));
  return f;
}

// LayerNorm is invariant to a shift along the features: fold the mean subtraction of the LayerNorm that follows a Linear
// into the Linear ((I - 11^T/n) W, (I - 11^T/n) b).  W is [n_out][n_in] row-major.
inline void center_outputs(std::vector<float> &W, std::vector<float> &b, int n_out, int n_in) {
  for (int k = 0; k < n_in; ++k) {
    double m = 0;
    for (int o = 0; o < n_out; ++o) m += W[(size_t)o * n_in + k];
    m /= n_out;
    for (int o = 0; o < n_out; ++o) W[(size_t)o * n_in + k] = (float)((double)W[(size_t)o * n_in + k] - m);
  }
  double mb = 0;
  for (int o = 0; o < n_out; ++o) mb += b[o];
  mb /= n_out;
  for (int o = 0; o < n_out; ++o) b[o] = (float)((double)b[o] - mb);
}

// conv weight [co][ci][k] -> [ci][k][co]
inline std::vector<float> conv_t(const float *w, int co, int ci, int k) {
  std::vector<float> t((size_t)co * ci * k, 0.f);
  if (!w) return t;
  for (int o = 0; o < co; ++o)
    for (int i = 0; i < ci; ++i)
      for (int d = 0; d < k; ++d) t[((size_t)i * k + d) * co + o] = w[((size_t)o * ci + i) * k + d];
  return t;
}

// conv weight [co][ci][k] (torch layout) -> A-operand fragments of v_mfma_f32_16x16x32_bf16 for the GEMM of actor_mfma_kernels.hip:
// [m-tile co/16][k-step][part hi, mid, lo][lane 64][4 dwords] (w = hi + mid + lo exactly, three bf16 parts); lane (r, q) holds row
// co = 16 mt + r, k-slots 8 q + (0..7) of the step, dword d = slots 2 d, 2 d + 1; GEMM index k = dk * ci_pad + ci (ci_pad = ci
// rounded up to a power of two >= 16; zeros beyond).
inline std::vector<float> pack_conv_frag(const float *w, int co, int ci, int ksz, int cp_force = 0, int co_pad = 0) {
  int cp = 16;
  while (cp < ci) cp *= 2;
  if (cp_force) cp = cp_force;     // Linear layers: ci itself (a multiple of 32); co_pad: output rows rounded up to 16 (zero rows)
  const int ks = (ksz * cp + 31) / 32, mts = (co_pad > co ? co_pad : co) / 16;
  std::vector<uint32_t> t((size_t)mts * ks * 768, 0u);
  if (w)
    for (int mt = 0; mt < mts; ++mt)
      for (int s = 0; s < ks; ++s)
        for (int lane = 0; lane < 64; ++lane)
          for (int d = 0; d < 4; ++d) {
            uint32_t part[3] = {0, 0, 0};
            for (int e = 0; e < 2; ++e) {
              const int k = s * 32 + 8 * (lane >> 4) + 2 * d + e;
              const int dk = k / cp, c = k % cp, o = 16 * mt + (lane & 15);
              float x = (dk < ksz && c < ci && o < co) ? w[((size_t)o * ci + c) * ksz + dk] : 0.f;
              for (int pi = 0; pi < 3; ++pi) {
                const uint16_t h = bf16_rne(x);
                part[pi] |= (uint32_t)h << (16 * e);
                x -= bf16_to_f32(h);
              }
            }
            const size_t base = ((size_t)(mt * ks + s) * 3) * 256 + (size_t)lane * 4 + d;
            for (int pi = 0; pi < 3; ++pi) t[base + 256 * pi] = part[pi];
          }
  std::vector<float> out(t.size());
  memcpy(out.data(), t.data(), t.size() * sizeof(float));
  return out;
}

// conv weight [co][ci][k] (torch layout) -> A-operand fragments of v_mfma_f32_16x16x4_f32 for the GEMM of actor_f32_kernels.hip:
// [m-tile co/16][k-group of 16][lane 64][4 floats]; lane (r, q) holds row co = 16 mt + r, GEMM indices k = 16 g + 4 q + (0..3),
// k = dk * ci_pad + ci (ci_pad = ci rounded up to a power of two >= 16; zeros beyond)
inline std::vector<float> pack_conv_f32(const float *w, int co, int ci, int ksz) {
  int cp = 16;
  while (cp < ci) cp *= 2;
  const int G = ksz * cp / 16, mts = co / 16;
  std::vector<float> t((size_t)mts * G * 256, 0.f);
  if (w)
    for (int mt = 0; mt < mts; ++mt)
      for (int g = 0; g < G; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int m = 0; m < 4; ++m) {
            const int k = g * 16 + 4 * (lane >> 4) + m;
            const int dk = k / cp, cc = k % cp, o = 16 * mt + (lane & 15);
            t[((size_t)(mt * G + g) * 64 + lane) * 4 + m] = (dk < ksz && cc < ci) ? w[((size_t)o * ci + cc) * ksz + dk] : 0.f;
          }
  return t;
}

// -------------------------------------------------------------------------------------------------
// wp_pack: state_dict -> blob, one function per network.  The order of the B.add calls IS the blob layout.
// -------------------------------------------------------------------------------------------------
// Linear @idx (transposed) + LayerNorm @idx+1
inline void wp_lin_ln(SD &sd, WeightBlob &B, const std::string &key, const std::string &p, int idx, int n_out, int n_in) {
  B.add(key + ".W", transpose(sd.get(p + "." + std::to_string(idx) + ".weight", (int64_t)n_out * n_in), n_out, n_in));
  B.add(key + ".b", vec(sd.get(p + "." + std::to_string(idx) + ".bias", n_out), n_out));
  B.add(key + ".g", vec(sd.get(p + "." + std::to_string(idx + 1) + ".weight", n_out), n_out));
  B.add(key + ".be", vec(sd.get(p + "." + std::to_string(idx + 1) + ".bias", n_out), n_out));
}

inline void wp_pack_lane(SD &sd, WeightBlob &B) {
  wp_lin_ln(sd, B, "lane.proj", "lane_net.proj", 0, 128, 16);
  for (int b = 0; b < 2; ++b) {
    std::string p = "lane_net.aggre" + std::to_string(b + 1), k = "lane.a" + std::to_string(b);
    wp_lin_ln(sd, B, k + ".f10", p + ".fc1", 0, 128, 128);
    wp_lin_ln(sd, B, k + ".f13", p + ".fc1", 3, 128, 128);
    wp_lin_ln(sd, B, k + ".f20", p + ".fc2", 0, 128, 256);
    wp_lin_ln(sd, B, k + ".f23", p + ".fc2", 3, 128, 128);
    B.add(k + ".ng", vec(sd.get(p + ".norm.weight", 128), 128));
    B.add(k + ".nb", vec(sd.get(p + ".norm.bias", 128), 128));
  }
}

// residual block r of the ActorNet has a downsample path: the first block of each of the four groups (not their second, not the output block)
inline bool wp_res_has_ds(int r) { return r < 8 && r % 2 == 0; }

inline void wp_pack_actor(SD &sd, WeightBlob &B) {
  const int chans[4] = {32, 64, 128, 256};
  int n_in = 14;
  int ri = 0;
  auto res = [&](const std::string &p, int ci, int co) {
    const bool ds = wp_res_has_ds(ri);
    std::string k = "act.r" + std::to_string(ri++);
    B.add(k + ".c1", conv_t(sd.get(p + ".conv1.weight", (int64_t)co * ci * 3), co, ci, 3));
    B.add(k + ".c2", conv_t(sd.get(p + ".conv2.weight", (int64_t)co * co * 3), co, co, 3));
    B.add(k + ".c1B", pack_conv_frag(sd.get(p + ".conv1.weight", (int64_t)co * ci * 3), co, ci, 3));
    B.add(k + ".c2B", pack_conv_frag(sd.get(p + ".conv2.weight", (int64_t)co * co * 3), co, co, 3));
    B.add(k + ".c1F", pack_conv_f32(sd.get(p + ".conv1.weight", (int64_t)co * ci * 3), co, ci, 3));
    B.add(k + ".c2F", pack_conv_f32(sd.get(p + ".conv2.weight", (int64_t)co * co * 3), co, co, 3));
    B.add(k + ".g1", vec(sd.get(p + ".bn1.weight", co), co));
    B.add(k + ".b1", vec(sd.get(p + ".bn1.bias", co), co));
    B.add(k + ".g2", vec(sd.get(p + ".bn2.weight", co), co));
    B.add(k + ".b2", vec(sd.get(p + ".bn2.bias", co), co));
    if (ds) {
      B.add(k + ".ds", conv_t(sd.get(p + ".downsample.0.weight", (int64_t)co * ci), co, ci, 1));
      B.add(k + ".dsB", pack_conv_frag(sd.get(p + ".downsample.0.weight", (int64_t)co * ci), co, ci, 1));
      B.add(k + ".dsF", pack_conv_f32(sd.get(p + ".downsample.0.weight", (int64_t)co * ci), co, ci, 1));
      B.add(k + ".gd", vec(sd.get(p + ".downsample.1.weight", co), co));
      B.add(k + ".bd", vec(sd.get(p + ".downsample.1.bias", co), co));
    }
  };
  for (int g = 0; g < 4; ++g) {
    res("actor_net.groups." + std::to_string(g) + ".0", n_in, chans[g]);
    res("actor_net.groups." + std::to_string(g) + ".1", chans[g], chans[g]);
    n_in = chans[g];
  }
  res("actor_net.output", 128, 128);
  for (int g = 0; g < 4; ++g) {
    std::string p = "actor_net.lateral." + std::to_string(g), k = "act.lat" + std::to_string(g);
    B.add(k + ".W", conv_t(sd.get(p + ".conv.weight", (int64_t)128 * chans[g] * 3), 128, chans[g], 3));
    B.add(k + ".WB", pack_conv_frag(sd.get(p + ".conv.weight", (int64_t)128 * chans[g] * 3), 128, chans[g], 3));
    B.add(k + ".WF", pack_conv_f32(sd.get(p + ".conv.weight", (int64_t)128 * chans[g] * 3), 128, chans[g], 3));
    B.add(k + ".g", vec(sd.get(p + ".norm.weight", 128), 128));
    B.add(k + ".b", vec(sd.get(p + ".norm.bias", 128), 128));
  }
}

inline void wp_pack_fusion(SD &sd, WeightBlob &B) {
  wp_lin_ln(sd, B, "fus.pa", "fusion_net.proj_actor", 0, 128, 128);
  wp_lin_ln(sd, B, "fus.pl", "fusion_net.proj_lane", 0, 128, 128);
  B.add("fus.pa.WM", pack_afrag(sd.get("fusion_net.proj_actor.0.weight", 128 * 128), 128));      // the same as fp32 MFMA A fragments (k_token_mfma)
  B.add("fus.pl.WM", pack_afrag(sd.get("fusion_net.proj_lane.0.weight", 128 * 128), 128));
  B.add("fus.pa.WB", pack_tok_bfrag(sd.get("fusion_net.proj_actor.0.weight", 128 * 128), 128));     // ... and as bf16 hi / lo fragments (k_token_mfma<1>)
  B.add("fus.pl.WB", pack_tok_bfrag(sd.get("fusion_net.proj_lane.0.weight", 128 * 128), 128));
  {
    // rpe table [32 chunks][8][4]: k<5 W_r[f][k], 5 bias, 6 gamma, 7 beta, f = 4 chunk + w
    const float *W = sd.get("fusion_net.proj_rpe_scene.0.weight", 128 * 5);
    const float *b = sd.get("fusion_net.proj_rpe_scene.0.bias", 128);
    const float *g = sd.get("fusion_net.proj_rpe_scene.1.weight", 128);
    const float *be = sd.get("fusion_net.proj_rpe_scene.1.bias", 128);
    std::vector<float> t(1024, 0.f);
    if (W && b && g && be)
      for (int ch = 0; ch < 32; ++ch)
        for (int w = 0; w < 4; ++w) {
          const int f = 4 * ch + w;
          for (int k = 0; k < 5; ++k) t[ch * 32 + k * 4 + w] = W[f * 5 + k];
          t[ch * 32 + 20 + w] = b[f];
          t[ch * 32 + 24 + w] = g[f];
          t[ch * 32 + 28 + w] = be[f];
        }
    B.add("fus.rtab", t);
  }
  for (int L = 0; L < 6; ++L) {
    std::string p = "fusion_net.fuse_scene.fusion." + std::to_string(L), k = "fus.L" + std::to_string(L);
    // proj_memory / proj_edge are followed by a LayerNorm: its mean subtraction is folded into the weights (center_outputs)
    std::vector<float> Wmc = vec(sd.get(p + ".proj_memory.0.weight", 128 * 384), 128 * 384);
    std::vector<float> bmc = vec(sd.get(p + ".proj_memory.0.bias", 128), 128);
    center_outputs(Wmc, bmc, 128, 384);
    const float *Wm = Wmc.data();
    B.add(k + ".WAe", pack_afrag(Wm, 384));
    B.add(k + ".WBe", pack_bfrag(Wmc, 384));
    B.add(k + ".WLe", pack_bfrag_lo3(Wmc, 384));
    B.add(k + ".WsT", transpose(Wm, 128, 128, 384, 128));
    B.add(k + ".WtT", transpose(Wm, 128, 128, 384, 256));
    B.add(k + ".bm", bmc);
    std::vector<float> vt(VT_SIZE, 0.f);
    auto put = [&](int off, const float *src) {
      if (src) memcpy(vt.data() + off, src, 128 * sizeof(float));
    };
    put(VT_GM, sd.get(p + ".proj_memory.1.weight", 128));
    put(VT_BM, sd.get(p + ".proj_memory.1.bias", 128));
    if (L != 5) {
      std::vector<float> Wpc = vec(sd.get(p + ".proj_edge.0.weight", 128 * 128), 128 * 128);
      std::vector<float> bpc = vec(sd.get(p + ".proj_edge.0.bias", 128), 128);
      center_outputs(Wpc, bpc, 128, 128);
      B.add(k + ".WAp", pack_afrag(Wpc.data(), 128));
      B.add(k + ".WBp", pack_bfrag(Wpc, 128));
      B.add(k + ".WLp", pack_bfrag_lo3(Wpc, 128));
      put(VT_BP, bpc.data());
      put(VT_GP, sd.get(p + ".proj_edge.1.weight", 128));
      put(VT_BEP, sd.get(p + ".proj_edge.1.bias", 128));
      put(VT_GE, sd.get(p + ".norm_edge.weight", 128));
      put(VT_BE, sd.get(p + ".norm_edge.bias", 128));
    }
    B.add(k + ".vtab", vt);
    const float *Win = sd.get(p + ".multihead_attn.in_proj_weight", 384 * 128);
    const float *bin = sd.get(p + ".multihead_attn.in_proj_bias", 384);
    {
      // the token kernel's projections as fp32 MFMA A fragments (k_token_mfma)
      const float *Wo_ = sd.get(p + ".multihead_attn.out_proj.weight", 128 * 128);
      const float *W1_ = sd.get(p + ".linear1.weight", 256 * 128), *W2_ = sd.get(p + ".linear2.weight", 128 * 256);
      B.add(k + ".WsM", pack_afrag(Wm + 128, 384));
      B.add(k + ".WtM", pack_afrag(Wm + 256, 384));
      B.add(k + ".WqM", pack_afrag(Win, 128));
      B.add(k + ".WkM", pack_wk_frag(Win ? Win + 128 * 128 : nullptr));
      B.add(k + ".WvM", pack_afrag(Win ? Win + 2 * 128 * 128 : nullptr, 128));
      B.add(k + ".WoM", pack_afrag(Wo_, 128));
      B.add(k + ".W1aM", pack_afrag(W1_, 128));
      B.add(k + ".W1bM", pack_afrag(W1_ ? W1_ + 128 * 128 : nullptr, 128));
      B.add(k + ".W2aM", pack_afrag(W2_, 256));
      B.add(k + ".W2bM", pack_afrag(W2_ ? W2_ + 128 : nullptr, 256));
      // ... and as bf16 hi / lo A fragments (k_token_mfma<1>; the folded K query keeps the fp32 fragments)
      B.add(k + ".WsB", pack_tok_bfrag(Wm + 128, 384));
      B.add(k + ".WtB", pack_tok_bfrag(Wm + 256, 384));
      B.add(k + ".WqB", pack_tok_bfrag(Win, 128));
      B.add(k + ".WvB", pack_tok_bfrag(Win ? Win + 2 * 128 * 128 : nullptr, 128));
      B.add(k + ".WoB", pack_tok_bfrag(Wo_, 128));
      B.add(k + ".W1aB", pack_tok_bfrag(W1_, 128));
      B.add(k + ".W1bB", pack_tok_bfrag(W1_ ? W1_ + 128 * 128 : nullptr, 128));
      B.add(k + ".W2aB", pack_tok_bfrag(W2_, 256));
      B.add(k + ".W2bB", pack_tok_bfrag(W2_ ? W2_ + 128 : nullptr, 256));
    }
    B.add(k + ".WqT", transpose(Win, 128, 128));
    B.add(k + ".Wk", vec(Win ? Win + 128 * 128 : nullptr, 128 * 128));
    B.add(k + ".WvT", transpose(Win ? Win + 2 * 128 * 128 : nullptr, 128, 128));
    B.add(k + ".bq", vec(bin, 128));
    B.add(k + ".bv", vec(bin ? bin + 256 : nullptr, 128));
    B.add(k + ".WoT", transpose(sd.get(p + ".multihead_attn.out_proj.weight", 128 * 128), 128, 128));
    B.add(k + ".bo", vec(sd.get(p + ".multihead_attn.out_proj.bias", 128), 128));
    B.add(k + ".W1T", transpose(sd.get(p + ".linear1.weight", 256 * 128), 256, 128));
    B.add(k + ".b1", vec(sd.get(p + ".linear1.bias", 256), 256));
    B.add(k + ".W2T", transpose(sd.get(p + ".linear2.weight", 128 * 256), 128, 256));
    B.add(k + ".b2", vec(sd.get(p + ".linear2.bias", 128), 128));
    B.add(k + ".g2", vec(sd.get(p + ".norm2.weight", 128), 128));
    B.add(k + ".be2", vec(sd.get(p + ".norm2.bias", 128), 128));
    B.add(k + ".g3", vec(sd.get(p + ".norm3.weight", 128), 128));
    B.add(k + ".be3", vec(sd.get(p + ".norm3.bias", 128), 128));
  }
}

inline void wp_pack_decoder(SD &sd, WeightBlob &B) {
  wp_lin_ln(sd, B, "dec.rpe", "pred_scene.proj_rpe", 0, 128, 20);
  wp_lin_ln(sd, B, "dec.t0", "pred_scene.proj_tgt", 0, 128, 256);
  wp_lin_ln(sd, B, "dec.t3", "pred_scene.proj_tgt", 3, 128, 128);
  wp_lin_ln(sd, B, "dec.c0", "pred_scene.ctx_proj", 0, 384, 128);
  wp_lin_ln(sd, B, "dec.c3", "pred_scene.ctx_proj", 3, 768, 384);
  wp_lin_ln(sd, B, "dec.a0", "pred_scene.actor_proj", 0, 384, 128);
  wp_lin_ln(sd, B, "dec.a3", "pred_scene.actor_proj", 3, 768, 384);
  B.add("dec.a0.WB", pack_conv_frag(sd.get("pred_scene.actor_proj.0.weight", 384 * 128), 384, 128, 1, 128));
  B.add("dec.a3.WB", pack_conv_frag(sd.get("pred_scene.actor_proj.3.weight", 768 * 384), 768, 384, 1, 384));
  B.add("dec.reg0.WB", pack_conv_frag(sd.get("pred_scene.reg.0.weight", 128 * 128), 128, 128, 1, 128));
  B.add("dec.reg3.WB", pack_conv_frag(sd.get("pred_scene.reg.3.weight", 128 * 128), 128, 128, 1, 128));
  B.add("dec.reg6.WB", pack_conv_frag(sd.get("pred_scene.reg.6.weight", 40 * 128), 40, 128, 1, 128, 48));
  {
    std::vector<float> b6 = vec(sd.get("pred_scene.reg.6.bias", 40), 40);
    b6.resize(48, 0.f);
    B.add("dec.reg6.bB", b6);
  }
  for (int L = 0; L < 2; ++L) {
    std::string p = "pred_scene.ctx_sat.layers." + std::to_string(L), k = "dec.e" + std::to_string(L);
    B.add(k + ".inW", transpose(sd.get(p + ".self_attn.in_proj_weight", 384 * 128), 384, 128));
    B.add(k + ".inb", vec(sd.get(p + ".self_attn.in_proj_bias", 384), 384));
    B.add(k + ".outW", transpose(sd.get(p + ".self_attn.out_proj.weight", 128 * 128), 128, 128));
    B.add(k + ".outb", vec(sd.get(p + ".self_attn.out_proj.bias", 128), 128));
    B.add(k + ".l1W", transpose(sd.get(p + ".linear1.weight", 1536 * 128), 1536, 128));
    B.add(k + ".l1b", vec(sd.get(p + ".linear1.bias", 1536), 1536));
    B.add(k + ".l2W", transpose(sd.get(p + ".linear2.weight", 128 * 1536), 128, 1536));
    B.add(k + ".l2b", vec(sd.get(p + ".linear2.bias", 128), 128));
    B.add(k + ".n1g", vec(sd.get(p + ".norm1.weight", 128), 128));
    B.add(k + ".n1b", vec(sd.get(p + ".norm1.bias", 128), 128));
    B.add(k + ".n2g", vec(sd.get(p + ".norm2.weight", 128), 128));
    B.add(k + ".n2b", vec(sd.get(p + ".norm2.bias", 128), 128));
  }
  for (const char *hn : {"cls", "reg"}) {
    std::string p = std::string("pred_scene.") + hn, k = std::string("dec.") + hn;
    wp_lin_ln(sd, B, k + "0", p, 0, 128, 128);
    wp_lin_ln(sd, B, k + "3", p, 3, 128, 128);
    const int nl = strcmp(hn, "cls") == 0 ? 1 : 40;
    B.add(k + "6.W", transpose(sd.get(p + ".6.weight", (int64_t)nl * 128), nl, 128));
    B.add(k + "6.b", vec(sd.get(p + ".6.bias", nl), nl));
  }
}

// The decoder's curve bases at the times ts (fractions of the horizon): float64 as numpy evaluates them -> fp32 (Q21).  T [n][8], Tp [n][7].
// basis 0: Bezier (network.py:449-464), T = C(7,i) (1-ts)^(7-i) ts^i, Tp = 7 C(6,i) (1-ts)^(6-i) ts^i
// basis 1: monomial (network.py:466-481), T = ts^i, Tp = (i+1) ts^i
#define WP_BASIS_BEZIER 0
#define WP_BASIS_MONOMIAL 1
inline void wp_basis_rows(int basis, const double *ts, int n, float *T, float *Tp) {
  auto comb = [](int n, int k) { double r = 1; for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i; return r; };
  for (int t = 0; t < n; ++t) {
    const double s = ts[t];
    if (basis == WP_BASIS_MONOMIAL) {
      for (int i = 0; i < 8; ++i) T[t * 8 + i] = (float)std::pow(s, i);
      for (int i = 0; i < 7; ++i) Tp[t * 7 + i] = (float)((double)(i + 1) * std::pow(s, i));
    } else {
      for (int i = 0; i < 8; ++i) T[t * 8 + i] = (float)(comb(7, i) * std::pow(1.0 - s, 7 - i) * std::pow(s, i));
      for (int i = 0; i < 7; ++i) Tp[t * 7 + i] = (float)(7.0 * comb(6, i) * std::pow(1.0 - s, 6 - i) * std::pow(s, i));
    }
  }
}

// the decoder's own time grid: numpy linspace(0, 1, 60) = start + arange * step, step = 1/59; last point exactly 1
inline void wp_basis_grid(double ts[60]) {
  for (int t = 0; t < 60; ++t) ts[t] = (t == 59) ? 1.0 : 0.0 + (double)t * (1.0 / 59.0);
}

// the tables of `basis` on the decoder's grid, written over the blob entries dec.T / dec.Tp (same shapes in both bases: no key, no offset moves)
inline void wp_basis_tables(int basis, float *T /*[60][8]*/, float *Tp /*[60][7]*/) {
  double ts[60];
  wp_basis_grid(ts);
  wp_basis_rows(basis, ts, 60, T, Tp);
}

// the default load packs the Bezier basis
inline void wp_pack_basis(WeightBlob &B) {
  std::vector<float> T(60 * 8), Tp(60 * 7);
  wp_basis_tables(WP_BASIS_BEZIER, T.data(), Tp.data());
  B.add("dec.T", T);
  B.add("dec.Tp", Tp);
}

// a tensor that is absent or has the wrong size is named in sd.missing (the first one); its entries are packed as zeros so the layout stands
inline void wp_pack(SD &sd, WeightBlob &B) {
  wp_pack_lane(sd, B);
  wp_pack_actor(sd, B);
  wp_pack_fusion(sd, B);
  wp_pack_decoder(sd, B);
  wp_pack_basis(B);
}

// -------------------------------------------------------------------------------------------------
// wp_bind: blob keys -> pointer tables
// -------------------------------------------------------------------------------------------------
struct WpLookup {
  const WeightBlob &B;
  const float *base;
  std::string missing;      // the first required key the blob does not hold
  // an entry the kernels read unconditionally
  const float *req(const std::string &k) {
    auto it = B.off.find(k);
    if (it != B.off.end()) return base + it->second;
    if (missing.empty()) missing = k;
    return nullptr;
  }
  // an entry the network does not have everywhere -- null where absent, and the kernels test for it: the downsample path of a residual block
  // (wp_res_has_ds), proj_edge of the last fusion layer
  const float *opt(const std::string &k) const {
    auto it = B.off.find(k);
    return it == B.off.end() ? nullptr : base + it->second;
  }
};

// residual block r in the packing `sfx` ("": transposed for the VALU kernel, "B": bf16 fragments, "F": fp32 fragments); Res = ResW / AmRes / AfRes
template <class Res>
inline void wp_bind_res(WpLookup &P, int r, const char *sfx, Res &R) {
  const std::string k = "act.r" + std::to_string(r);
  const bool ds = wp_res_has_ds(r);
  auto get = [&](const std::string &key) { return ds ? P.req(key) : P.opt(key); };
  R.c1 = (decltype(R.c1))P.req(k + ".c1" + sfx); R.g1 = P.req(k + ".g1"); R.b1 = P.req(k + ".b1");
  R.c2 = (decltype(R.c2))P.req(k + ".c2" + sfx); R.g2 = P.req(k + ".g2"); R.b2 = P.req(k + ".b2");
  R.ds = (decltype(R.ds))get(k + ".ds" + sfx); R.gd = get(k + ".gd"); R.bd = get(k + ".bd");
}

// lateral conv g in the packing `sfx`
template <class Wt>
inline void wp_bind_lat(WpLookup &P, int g, const char *sfx, const Wt *&w, const float *&gamma, const float *&beta) {
  const std::string k = "act.lat" + std::to_string(g);
  w = (const Wt *)P.req(k + ".W" + sfx); gamma = P.req(k + ".g"); beta = P.req(k + ".b");
}

// token table L of 7: the epilogue of fusion layer L-1 and the prologue of layer L; the halves that fall off either end of the six layers stay null
inline void wp_bind_tok(WpLookup &P, int L, TokWeights &w) {
  if (L >= 1) {
    std::string k = "fus.L" + std::to_string(L - 1);
    w.WvT = P.req(k + ".WvT"); w.bv = P.req(k + ".bv"); w.WoT = P.req(k + ".WoT"); w.bo = P.req(k + ".bo");
    w.g2 = P.req(k + ".g2"); w.b2 = P.req(k + ".be2"); w.W1T = P.req(k + ".W1T"); w.b1 = P.req(k + ".b1");
    w.W2T = P.req(k + ".W2T"); w.bb2 = P.req(k + ".b2"); w.g3 = P.req(k + ".g3"); w.b3 = P.req(k + ".be3");
  }
  if (L <= 5) {
    std::string k = "fus.L" + std::to_string(L);
    w.WsT = P.req(k + ".WsT"); w.WtT = P.req(k + ".WtT"); w.bm = P.req(k + ".bm");
    w.WqT = P.req(k + ".WqT"); w.bq = P.req(k + ".bq"); w.Wk = P.req(k + ".Wk");
  }
  w.WpaT = P.req("fus.pa.W"); w.bpa = P.req("fus.pa.b"); w.gpa = P.req("fus.pa.g"); w.bepa = P.req("fus.pa.be");
  w.WplT = P.req("fus.pl.W"); w.bpl = P.req("fus.pl.b"); w.gpl = P.req("fus.pl.g"); w.bepl = P.req("fus.pl.be");
}

// ... the same matrices as A fragments, sfx "M" (fp32) or "B" (bf16 hi / lo); the folded K query keeps the fp32 fragments in both
inline void wp_bind_tok_frag(WpLookup &P, int L, const char *sfx, TokWeightsM &m) {
  if (L >= 1) {
    std::string k = "fus.L" + std::to_string(L - 1);
    m.Wv = P.req(k + ".Wv" + sfx); m.Wo = P.req(k + ".Wo" + sfx); m.W1a = P.req(k + ".W1a" + sfx); m.W1b = P.req(k + ".W1b" + sfx);
    m.W2a = P.req(k + ".W2a" + sfx); m.W2b = P.req(k + ".W2b" + sfx);
  }
  if (L <= 5) {
    std::string k = "fus.L" + std::to_string(L);
    m.Ws = P.req(k + ".Ws" + sfx); m.Wt = P.req(k + ".Wt" + sfx); m.Wq = P.req(k + ".Wq" + sfx); m.Wkf = P.req(k + ".WkM");
  }
  m.Wpa = P.req(std::string("fus.pa.W") + sfx); m.Wpl = P.req(std::string("fus.pl.W") + sfx);
}

// fills T with base + offset of every entry the kernels read.  False when a required key is absent (*missing: the first one); T is then not to be used.
inline bool wp_bind(const WeightBlob &B, const float *base, WeightTables &T, std::string *missing) {
  WpLookup P{B, base, {}};
  T = WeightTables{};
  LaneW &lw = T.lane;
  lw.pW = P.req("lane.proj.W"); lw.pb = P.req("lane.proj.b"); lw.pg = P.req("lane.proj.g"); lw.pbe = P.req("lane.proj.be");
  for (int b = 0; b < 2; ++b) {
    std::string k = "lane.a" + std::to_string(b);
    lw.f10W[b] = P.req(k + ".f10.W"); lw.f10b[b] = P.req(k + ".f10.b"); lw.f10g[b] = P.req(k + ".f10.g"); lw.f10be[b] = P.req(k + ".f10.be");
    lw.f13W[b] = P.req(k + ".f13.W"); lw.f13b[b] = P.req(k + ".f13.b"); lw.f13g[b] = P.req(k + ".f13.g"); lw.f13be[b] = P.req(k + ".f13.be");
    lw.f20W[b] = P.req(k + ".f20.W"); lw.f20b[b] = P.req(k + ".f20.b"); lw.f20g[b] = P.req(k + ".f20.g"); lw.f20be[b] = P.req(k + ".f20.be");
    lw.f23W[b] = P.req(k + ".f23.W"); lw.f23b[b] = P.req(k + ".f23.b"); lw.f23g[b] = P.req(k + ".f23.g"); lw.f23be[b] = P.req(k + ".f23.be");
    lw.ng[b] = P.req(k + ".ng"); lw.nbe[b] = P.req(k + ".nb");
  }
  for (int r = 0; r < 9; ++r) {
    wp_bind_res(P, r, "", T.actor.res[r]);
    wp_bind_res(P, r, "B", T.actorB.res[r]);
    wp_bind_res(P, r, "F", T.actorF.res[r]);
  }
  for (int g = 0; g < 4; ++g) {
    wp_bind_lat(P, g, "", T.actor.latW[g], T.actor.latG[g], T.actor.latB[g]);
    wp_bind_lat(P, g, "B", T.actorB.lat[g].w, T.actorB.lat[g].g, T.actorB.lat[g].b);
    wp_bind_lat(P, g, "F", T.actorF.lat[g].w, T.actorF.lat[g].g, T.actorF.lat[g].b);
  }
  PairW &pw = T.pair;
  pw.rtab = P.req("fus.rtab");
  for (int L = 0; L < 6; ++L) {
    std::string k = "fus.L" + std::to_string(L);
    auto edge = [&](const std::string &key) { return L != 5 ? P.req(key) : P.opt(key); };     // the last layer has no proj_edge
    pw.WAe[L] = P.req(k + ".WAe");
    pw.WAp[L] = edge(k + ".WAp");
    pw.WBe[L] = (const u32 *)P.req(k + ".WBe");
    pw.WBp[L] = (const u32 *)edge(k + ".WBp");
    pw.WLe[L] = (const u32 *)P.req(k + ".WLe");
    pw.WLp[L] = (const u32 *)edge(k + ".WLp");
    pw.vtab[L] = P.req(k + ".vtab");
  }
  for (int L = 0; L <= 6; ++L) {
    wp_bind_tok(P, L, T.tok[L]);
    wp_bind_tok_frag(P, L, "M", T.tokM[L]);
    wp_bind_tok_frag(P, L, "B", T.tokB[L]);
  }
  DecW &d = T.dec;
  d.rpeW = P.req("dec.rpe.W"); d.rpeb = P.req("dec.rpe.b"); d.rpeg = P.req("dec.rpe.g"); d.rpebe = P.req("dec.rpe.be");
  d.t0W = P.req("dec.t0.W"); d.t0b = P.req("dec.t0.b"); d.t0g = P.req("dec.t0.g"); d.t0be = P.req("dec.t0.be");
  d.t3W = P.req("dec.t3.W"); d.t3b = P.req("dec.t3.b"); d.t3g = P.req("dec.t3.g"); d.t3be = P.req("dec.t3.be");
  d.c0W = P.req("dec.c0.W"); d.c0b = P.req("dec.c0.b"); d.c0g = P.req("dec.c0.g"); d.c0be = P.req("dec.c0.be");
  d.c3W = P.req("dec.c3.W"); d.c3b = P.req("dec.c3.b"); d.c3g = P.req("dec.c3.g"); d.c3be = P.req("dec.c3.be");
  d.a0W = P.req("dec.a0.W"); d.a0b = P.req("dec.a0.b"); d.a0g = P.req("dec.a0.g"); d.a0be = P.req("dec.a0.be");
  d.a3W = P.req("dec.a3.W"); d.a3b = P.req("dec.a3.b"); d.a3g = P.req("dec.a3.g"); d.a3be = P.req("dec.a3.be");
  for (int L = 0; L < 2; ++L) {
    std::string k = "dec.e" + std::to_string(L);
    d.inW[L] = P.req(k + ".inW"); d.inb[L] = P.req(k + ".inb"); d.outW[L] = P.req(k + ".outW"); d.outb[L] = P.req(k + ".outb");
    d.l1W[L] = P.req(k + ".l1W"); d.l1b[L] = P.req(k + ".l1b"); d.l2W[L] = P.req(k + ".l2W"); d.l2b[L] = P.req(k + ".l2b");
    d.n1g[L] = P.req(k + ".n1g"); d.n1b[L] = P.req(k + ".n1b"); d.n2g[L] = P.req(k + ".n2g"); d.n2b[L] = P.req(k + ".n2b");
  }
  d.k0W = P.req("dec.cls0.W"); d.k0b = P.req("dec.cls0.b"); d.k0g = P.req("dec.cls0.g"); d.k0be = P.req("dec.cls0.be");
  d.k3W = P.req("dec.cls3.W"); d.k3b = P.req("dec.cls3.b"); d.k3g = P.req("dec.cls3.g"); d.k3be = P.req("dec.cls3.be");
  d.k6W = P.req("dec.cls6.W"); d.k6b = P.req("dec.cls6.b");
  d.r0W = P.req("dec.reg0.W"); d.r0b = P.req("dec.reg0.b"); d.r0g = P.req("dec.reg0.g"); d.r0be = P.req("dec.reg0.be");
  d.r3W = P.req("dec.reg3.W"); d.r3b = P.req("dec.reg3.b"); d.r3g = P.req("dec.reg3.g"); d.r3be = P.req("dec.reg3.be");
  d.r6W = P.req("dec.reg6.W"); d.r6b = P.req("dec.reg6.b");
  d.T = P.req("dec.T"); d.Tp = P.req("dec.Tp");
  DmW &m = T.decB;
  m.a0 = (const u32 *)P.req("dec.a0.WB"); m.a3 = (const u32 *)P.req("dec.a3.WB"); m.r0 = (const u32 *)P.req("dec.reg0.WB");
  m.r3 = (const u32 *)P.req("dec.reg3.WB"); m.r6 = (const u32 *)P.req("dec.reg6.WB");
  m.a0b = d.a0b; m.a0g = d.a0g; m.a0be = d.a0be; m.a3b = d.a3b; m.a3g = d.a3g; m.a3be = d.a3be;
  m.r0b = d.r0b; m.r0g = d.r0g; m.r0be = d.r0be; m.r3b = d.r3b; m.r3g = d.r3g; m.r3be = d.r3be; m.r6b = P.req("dec.reg6.bB");
  m.T = d.T; m.Tp = d.Tp;
  if (missing) *missing = P.missing;
  return P.missing.empty();
}
