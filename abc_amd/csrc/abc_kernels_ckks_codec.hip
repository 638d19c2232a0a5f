// abc_kernels_ckks_codec.hip -- CKKS slot encoder / decoder on the device (abc_hip_ckks_encode / abc_hip_ckks_decode).
//
// The reference has no CKKS code (its BatchEncoder call sites are SealCiphertextFactory.cpp:130 / :151); the slot order is the
// one the CPU oracle's encoder and runtime/CkksEncoder.hpp use: slot i holds the evaluation of the real polynomial m(X) at
// zeta^g, g = 3^i mod 2N, zeta = exp(i pi / N).
//
// Half-size transform.  With M = N/2 write m(X) = A(X) + X^M B(X) (A, B real, degree < M) and u_k = m_k + i m_{k+M}, i.e.
// U(X) = A(X) + i B(X).  At a root x = zeta^(4l+1) (l < M), x^M = zeta^((4l+1) M) = i, so m(x) = U(x).  The N/2 roots of that
// form contain exactly one of every conjugate pair {zeta^g, zeta^-g}, so the slots fix U completely:
//   v_l = U(zeta omega^l),  omega = zeta^4 = exp(2 pi i / M),
//   slot i, g = 3^i mod 2N:   g = 1 mod 4 -> v_l = z_i with l = (g - 1) / 4
//                             g = 3 mod 4 -> v_l = conj(z_i) with l = (2N - g - 1) / 4      (m real: m(zeta^-g) = conj(m(zeta^g)))
// In terms of the oracle's position j = (g - 1) / 2 of slot i: l = j / 2 for even j, l = (N - 1 - j) / 2 (conjugated) for odd j.
//   encode (inverse direction):  u_k = zeta^-k / M * sum_l v_l omega^(-lk),   m_k = Re(u_k) * scale, m_{k+M} = Im(u_k) * scale
//   decode (forward direction):  v_l = sum_k (u_k zeta^k) omega^(lk),          u_k = (m_k + i m_{k+M}) / scale
// The table p2s[l] = i | conj << 31 (position -> slot) serves both: the encoder's first load gathers through it, the decoder's
// last store scatters through it.
//
// Transform layout: M complex doubles take 16 M bytes.
//   N <= 2^14 (M <= 8192, <= 128 KiB): one workgroup per polynomial, the whole transform resident in LDS.
//   N = 2^15 / 2^16: four-step, M = M1 x M2 with M2 = 128: pass 1 transforms the M2 columns (length M1, stride M2) and applies
//   the twiddle omega^(n2 k1), writing Y[k1 M2 + n2] to HBM; pass 2 transforms the rows of Y (length M2) and writes element
//   k1 + M1 k2.  Either pass holds 4096 points (64 KiB) per workgroup.
// Both directions are radix-2 Cooley-Tukey on bit-reversed LDS input; twiddles omega^k and the twist zeta^k come from tables
// built on the host in long double and uploaded once per context, on first use.
//
// Encode fusions: the first load gathers the slots (zero beyond values_per_row); the last store applies twist x scale / M,
// rounding (ties away from zero), the |c| < 2^62 range flag (one word, read back once per call) and the reduction into every limb, writing coefficient
// form; the existing forward NTT launcher then brings the plaintext into NTT form.
// Decode fusions: the existing inverse NTT runs into scratch; the first load does the Garner digits (per-limb constants), a
// multi-word Horner, the compare with Q/2 of the level (exact centred lift of any residue vector), the conversion to double,
// x 1/scale and the twist; the last store scatters into the slot vectors.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "abc_context.hpp"
#include "abc_crt_lift.hpp"
#include "abc_host_math.hpp"

namespace abc {
namespace {

struct alignas(16) cplx {
  double x, y;
};
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cmul_conj(cplx a, cplx b) { return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }  // a conj(b)

// per-context table block: omega[M], zeta[M], p2s[M]; the CRT constants of the lift are the context's (abc_crt_lift.hpp)
struct CodecTables {
  const cplx *omega, *zeta;
  const u32 *p2s;
  const CodecConst *k;
};
size_t tables_bytes(size_t M) { return M * 16 * 2 + M * 4; }
CodecTables tables_at(const abc_hip_ctx *c) {
  const size_t M = (size_t)c->n / 2;
  char *b = (char *)c->d_ckks_codec;
  return {(const cplx *)b, (const cplx *)(b + M * 16), (const u32 *)(b + M * 32), (const CodecConst *)c->d_crt};
}

int ensure_tables(abc_hip_ctx *c) {
  if (ensure_crt_const(c)) return 1;
  if (c->d_ckks_codec) return 0;
  const size_t N = (size_t)c->n, M = N / 2;
  std::vector<char> blk(tables_bytes(M), 0);
  cplx *omega = (cplx *)blk.data(), *zeta = (cplx *)(blk.data() + M * 16);
  u32 *p2s = (u32 *)(blk.data() + M * 32);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (size_t j = 0; j < M; ++j) {
    const long double a = 2 * pi * (long double)j / (long double)M, z = pi * (long double)j / (long double)N;
    omega[j] = {(double)cosl(a), (double)sinl(a)};
    zeta[j] = {(double)cosl(z), (double)sinl(z)};
  }
  uint64_t g = 1;
  for (size_t i = 0; i < M; ++i) {
    const size_t j = (size_t)(g - 1) >> 1;
    if (j & 1) p2s[(N - 1 - j) >> 1] = (u32)i | 0x80000000u;
    else p2s[j >> 1] = (u32)i;
    g = (g * 3) & (2 * N - 1);
  }
  void *d = nullptr;
  ABC_HIP_CHECK(hipMalloc(&d, blk.size()));
  if (hipMemcpy(d, blk.data(), blk.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    set_error("ckks codec: table upload failed");
    return 1;
  }
  c->d_ckks_codec = d;
  return 0;
}

// ---- the transform kernel ----
// kind 0: whole transform of length M = 2^log_len per workgroup (one line)
// kind 1: four-step pass 1: line n2 (of M2 = 2^log_m2), element n1 at n = n1 M2 + n2; stores Y[k1 M2 + n2] * omega^(sign n2 k1)
// kind 2: four-step pass 2: line k1, element n2 at Y[k1 M2 + n2]; stores element k1 + M1 k2
struct FftGeom {
  int kind, log_len, log_lines, log_m, log_m1, log_m2, sign;
};
constexpr int kThreads = 512;

template <class Src, class Dst>
__global__ __launch_bounds__(kThreads) void k_ckks_fft(Src src, Dst dst, FftGeom g, const cplx *__restrict__ omega) {
  extern __shared__ cplx sh[];  // [lines][len + 1]: the pad keeps line-strided accesses off one bank
  const int len = 1 << g.log_len, lines = 1 << g.log_lines, stride = len + 1, total = len << g.log_lines;
  const size_t b = blockIdx.y;
  const int base = (int)blockIdx.x << g.log_lines;
  for (int idx = threadIdx.x; idx < total; idx += kThreads) {
    int t, e;
    if (g.kind == 2) {  // rows of Y are contiguous: element-fast
      e = idx & (len - 1);
      t = idx >> g.log_len;
    } else {  // columns: line-fast (consecutive lines are consecutive words)
      t = idx & (lines - 1);
      e = idx >> g.log_lines;
    }
    const int line = base + t;
    const int n = g.kind == 0 ? e : g.kind == 1 ? (e << g.log_m2) + line : (line << g.log_m2) + e;
    sh[t * stride + (int)bitrev32((u32)e, g.log_len)] = src(b, n);
  }
  __syncthreads();
  const int half = total >> 1;
  for (int ls = 1; ls <= g.log_len; ++ls) {
    const int h = 1 << (ls - 1), tw_shift = g.log_m - ls;  // omega_(2h)^pos = omega_M^(pos << (log_m - ls))
    for (int bi = threadIdx.x; bi < half; bi += kThreads) {
      const int t = bi >> (g.log_len - 1), r = bi & ((len >> 1) - 1);
      const int pos = r & (h - 1), i0 = t * stride + ((r >> (ls - 1)) << ls) + pos, i1 = i0 + h;
      cplx w = omega[pos << tw_shift];
      if (g.sign < 0) w.y = -w.y;
      const cplx u = sh[i0], v = cmul(sh[i1], w);
      sh[i0] = {u.x + v.x, u.y + v.y};
      sh[i1] = {u.x - v.x, u.y - v.y};
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < total; idx += kThreads) {
    const int t = idx & (lines - 1), e = idx >> g.log_lines, line = base + t;
    const cplx v = sh[t * stride + e];
    if (g.kind == 0) {
      dst(b, e, v);
    } else if (g.kind == 1) {
      cplx w = omega[(line * e) & ((1 << g.log_m) - 1)];
      if (g.sign < 0) w.y = -w.y;
      dst(b, (e << g.log_m2) + line, cmul(v, w));
    } else {
      dst(b, line + (e << g.log_m1), v);
    }
  }
}

// four-step intermediate [count][M]
struct SrcY {
  const cplx *y;
  size_t M;
  __device__ cplx operator()(size_t b, int n) const { return y[b * M + n]; }
};
struct DstY {
  cplx *y;
  size_t M;
  __device__ void operator()(size_t b, int n, cplx v) const { y[b * M + n] = v; }
};

// encode, first load: v_l from the slot values of row b (zero beyond values_per_row)
struct SrcSlots {
  const double *re, *im;
  size_t vpr;
  const u32 *p2s;
  __device__ cplx operator()(size_t b, int l) const {
    const u32 e = p2s[l], i = e & 0x7fffffffu;
    cplx z{0.0, 0.0};
    if (i < vpr) {
      z.x = re[b * vpr + i];
      z.y = im ? im[b * vpr + i] : 0.0;
      if (e >> 31) z.y = -z.y;
    }
    return z;
  }
};

// encode, last store: twist, scale / M, round (ties away from zero), range flag, reduction into every limb (coefficient form, [count][nl][N])
struct DstCoef {
  DevCtx c;
  u64 *plain;
  int nl;
  size_t M;
  double f;  // scale / M
  const cplx *zeta;
  int *flag;
  __device__ void put(u64 *o, double x) const {
    const double r = __builtin_round(x);  // nearest, ties away from zero (abc_hip.h; abc_hip_ckks_const_words' rule)
    u64 mag = 0;
    bool neg = false;
    if (__builtin_fabs(r) < 0x1p62) {  // also false for NaN
      neg = r < 0;
      mag = (u64)__builtin_fabs(r);
    } else {
      atomicOr(flag, 1);
    }
    for (int j = 0; j < nl; ++j) {
      const Mod m = mod_at(c, j);
      const u64 v = reduce64(mag, m);
      o[(size_t)j * c.n] = neg ? neg_mod(v, m.q) : v;
    }
  }
  __device__ void operator()(size_t b, int k, cplx v) const {
    const cplx u = cmul_conj(v, zeta[k]);
    u64 *o = plain + b * nl * c.n + k;
    put(o, u.x * f);
    put(o + M, u.y * f);
  }
};

// decode, first load: exact centred lift of coefficients n and n + M (coefficient form in scratch), / scale, times zeta^n
template <int NLW>
struct SrcLift {
  DevCtx c;
  const u64 *coef;
  int nl;
  size_t M;
  double inv_scale;
  const cplx *zeta;
  const CodecConst *k;
  __device__ double lift(const u64 *p) const {  // p: limb 0 of the coefficient; limbs are N words apart
    const size_t n = (size_t)c.n;
    u64 x[NLW];
    const bool gt = crt_lift_centred<NLW>(c.mods, k, nl, [p, n](int j, const Mod &) { return p[(size_t)j * n]; }, x);
    double v = 0.0;
#pragma unroll
    for (int w = NLW - 1; w >= 0; --w) v = v * 0x1p64 + (double)x[w];
    return gt ? -v : v;
  }
  __device__ cplx operator()(size_t b, int n) const {
    const u64 *p = coef + b * nl * c.n + n;
    const cplx u{lift(p) * inv_scale, lift(p + M) * inv_scale};
    return cmul(u, zeta[n]);
  }
};

// decode, last store: position l -> slot (conjugated where the table says so), [count][M]
struct DstSlots {
  double *re, *im;
  size_t M;
  const u32 *p2s;
  __device__ void operator()(size_t b, int l, cplx v) const {
    const u32 e = p2s[l], i = e & 0x7fffffffu;
    re[b * M + i] = v.x;
    if (im) im[b * M + i] = (e >> 31) ? -v.y : v.y;
  }
};

size_t lds_bytes(const FftGeom &g) { return (size_t)((1 << g.log_len) + 1) * ((size_t)1 << g.log_lines) * sizeof(cplx); }

// one transform of `cc` polynomials: src -> dst, through the four-step intermediate Y where N > 2^14
template <class Src, class Dst>
int run_fft(abc_hip_ctx *c, const Src &src, const Dst &dst, cplx *Y, size_t cc, int sign, const CodecTables &t) {
  const int log_m = c->logn - 1;
  const size_t M = (size_t)1 << log_m;
  if (c->logn <= 14) {
    const FftGeom g{0, log_m, 0, log_m, log_m, 0, sign};
    hipLaunchKernelGGL((k_ckks_fft<Src, Dst>), dim3(1, (unsigned)cc), dim3(kThreads), lds_bytes(g), c->stream, src, dst, g, t.omega);
    ABC_HIP_CHECK(hipGetLastError());
    return 0;
  }
  const int log_m2 = 7, log_m1 = log_m - log_m2;  // 4096 points per workgroup in either pass
  const FftGeom g1{1, log_m1, 12 - log_m1, log_m, log_m1, log_m2, sign};
  const FftGeom g2{2, log_m2, 12 - log_m2, log_m, log_m1, log_m2, sign};
  hipLaunchKernelGGL((k_ckks_fft<Src, DstY>), dim3(1u << (log_m2 - g1.log_lines), (unsigned)cc), dim3(kThreads), lds_bytes(g1), c->stream,
                     src, DstY{Y, M}, g1, t.omega);
  ABC_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_ckks_fft<SrcY, Dst>), dim3(1u << (log_m1 - g2.log_lines), (unsigned)cc), dim3(kThreads), lds_bytes(g2), c->stream,
                     SrcY{Y, M}, dst, g2, t.omega);
  ABC_HIP_CHECK(hipGetLastError());
  return 0;
}

int check_args(abc_hip_ctx *c, const char *what, int nl, double scale) {
  if (c->scheme != 2) { set_error(std::string(what) + " needs a CKKS context"); return 1; }
  if (nl < 1 || nl > c->L) { set_error(std::string(what) + ": limb count out of range for this context"); return 1; }
  if (!(scale > 0) || !std::isfinite(scale)) { set_error(std::string(what) + ": scale must be positive and finite"); return 1; }
  return 0;
}

constexpr size_t kScratchCap = (size_t)256 << 20;  // bytes of per-chunk scratch a call asks the workspace for
constexpr size_t kMaxGridY = 65535;

}  // namespace

int ckks_encode(abc_hip_ctx *c, const double *re, const double *im, size_t vpr, double scale, int nl, u64 *plain, size_t count) {
  if (check_args(c, "ckks_encode", nl, scale)) return 1;
  const size_t N = (size_t)c->n, M = N / 2;
  if (vpr > M) { set_error("ckks_encode: values_per_row exceeds N/2 slots"); return 1; }
  if (vpr && !re) { set_error("ckks_encode: null values"); return 1; }
  if (!count) return 0;
  if (ensure_tables(c)) return 1;
  const CodecTables t = tables_at(c);
  const size_t per = c->logn > 14 ? M * sizeof(cplx) : 0;
  const size_t chunk = std::min({count, kMaxGridY, per ? std::max<size_t>(1, kScratchCap / per) : count});
  if (ensure_workspace(c, 256 + chunk * per)) return 1;
  int *flag = (int *)c->ws;
  cplx *Y = (cplx *)((char *)c->ws + 256);
  ABC_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
  for (size_t b0 = 0; b0 < count; b0 += chunk) {
    const size_t cc = std::min(chunk, count - b0);
    const SrcSlots src{re ? re + b0 * vpr : nullptr, im ? im + b0 * vpr : nullptr, vpr, t.p2s};
    const DstCoef dst{c->dc, plain + b0 * nl * N, nl, M, scale / (double)M, t.zeta, flag};
    if (run_fft(c, src, dst, Y, cc, -1, t)) return 1;
  }
  if (launch_ntt_fwd(c, plain, key_limb_map(c, nl), nl, count * nl)) return 1;
  int h = 0;
  ABC_HIP_CHECK(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ABC_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h) {
    set_error("ckks_encode: a scaled coefficient reaches 2^62 in magnitude (scale too large for these values, or a value is not finite)");
    return 2;
  }
  return 0;
}

int ckks_decode(abc_hip_ctx *c, const u64 *plain, int nl, double scale, double *re, double *im, size_t count) {
  if (check_args(c, "ckks_decode", nl, scale)) return 1;
  if (!count) return 0;
  if (!re) { set_error("ckks_decode: null output"); return 1; }
  if (ensure_tables(c)) return 1;
  const CodecTables t = tables_at(c);
  const size_t N = (size_t)c->n, M = N / 2;
  const size_t coef_bytes = (size_t)nl * N * 8, per = coef_bytes + (c->logn > 14 ? M * sizeof(cplx) : 0);
  const size_t chunk = std::min({count, kMaxGridY, std::max<size_t>(1, kScratchCap / per)});
  if (ensure_workspace(c, chunk * per)) return 1;
  u64 *coef = (u64 *)c->ws;
  cplx *Y = (cplx *)((char *)c->ws + chunk * coef_bytes);
  const LimbMap map = key_limb_map(c, nl);
  for (size_t b0 = 0; b0 < count; b0 += chunk) {
    const size_t cc = std::min(chunk, count - b0);
    ABC_HIP_CHECK(hipMemcpyAsync(coef, plain + b0 * nl * N, cc * coef_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (launch_ntt_inv(c, coef, map, nl, cc * nl)) return 1;
    const DstSlots dst{re + b0 * M, im ? im + b0 * M : nullptr, M, t.p2s};
    int rc;
    if (nl <= 4) rc = run_fft(c, SrcLift<4>{c->dc, coef, nl, M, 1.0 / scale, t.zeta, t.k}, dst, Y, cc, 1, t);
    else if (nl <= 8) rc = run_fft(c, SrcLift<8>{c->dc, coef, nl, M, 1.0 / scale, t.zeta, t.k}, dst, Y, cc, 1, t);
    else rc = run_fft(c, SrcLift<16>{c->dc, coef, nl, M, 1.0 / scale, t.zeta, t.k}, dst, Y, cc, 1, t);
    if (rc) return 1;
  }
  return 0;
}

}  // namespace abc
