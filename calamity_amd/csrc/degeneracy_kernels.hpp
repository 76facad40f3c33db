// degeneracy_kernels.hpp -- refer a fitted solution to a reference (sky) model (cal_solver_fix_degeneracies).  A fit constrains only
// g_i conj(g_j) m_b; per slice t and channel f an amplitude eta, a phase psi and a tilt Phi = (Phi_e, Phi_n) are free.  Baseline row b
// has antennas (i, j), d_b = r_i - r_j (east, north; metres), m = A c (MODE_MODEL's planes), s the reference, w its weights:
//   z0_b = (w > 0) w conj(m) s        in T            Q = sum_b (w > 0) w |m|^2       H = sum_b |z0_b| d_b d_b^T
//   z_b = z0_b e^{-i Phi.d_b},  q = sum_b Im(z_b) d_b,  Phi += H^+ q     (iters times, from Phi = 0)
//   e^{2 eta} = max(sum_b Re z_b, 0) / Q     at the last Phi
//   psi = arg sum_a g_a e^{-i Phi.r_a} conj(gref_a)    over the antennas with a cross-correlation row with w > 0, ascending
//   m' = m e^{2 eta} e^{i Phi.d_b},   g'_a = g_a e^{-eta} e^{-i (Phi.r_a + psi)}
// Six kernels behind the model pass:
//   degen_rows_kernel         once: z0 over the reference planes, in place
//   degen_sum_kernel          iters + 1 times: per segment of kDgSeg rows of a slice's row list and per channel, the sums in double
//   degen_solve_kernel        behind every sum: the segments' partials in a fixed order, then the step (or, last, the amplitude)
//   degen_phase_kernel        psi
//   degen_apply_gains_kernel  g'
//   degen_apply_rows_kernel   m', in place over the model planes
// Every sum over rows, antennas and channels is taken in double in an order the problem alone decides (a slice's rows ascending, cut
// every kDgSeg rows, the segments' sums added in kDgParts runs of neighbours; no atomics): two calls give the same bits, and a slice of a batch the bits of the same slice alone.
#pragma once
#include "row_walk.hpp"

namespace calk {

constexpr int kDgSeg = 128;  // rows per segment of degen_sum_kernel
constexpr int kDgParts = 8;  // waves of a block of degen_solve_kernel: each adds one run of the slice's segments
// the per-channel planes of the call's state, [kDgPlanes][nsl][fpad] doubles, followed by the band's Phi_0 [nsl][2]
enum { DG_Q = 0, DG_HEE, DG_HEN, DG_HNN, DG_CNT, DG_QE, DG_QN, DG_SRE, DG_PE, DG_PN, DG_STEP, DG_ETA, DG_PSI, DG_AMP2, kDgPlanes };
constexpr int kDgFirstSums = 8, kDgIterSums = 3;  // per segment: q_e, q_n, sum Re z (every launch) | Q, H_ee, H_en, H_nn, count (the first)
struct DgSeg { int slice, e0, e1, pad; };         // rows ent[e0 .. e1) of slice `slice`

// H^+ q for the symmetric 2x2 H = [a b; b c] (tr H > 0): the inverse where det H > 1e-12 (tr H / 2)^2, else -- the array is a line --
// the step along the dominant eigenvector alone.
__host__ __device__ inline void dg_step2(double a, double b, double c, double qe, double qn, double* se, double* sn) {
#pragma clang fp contract(off)
  const double tr = a + c, det = a * c - b * b, half = 0.5 * tr;
  if (det > 1e-12 * half * half) {
    *se = (c * qe - b * qn) / det;
    *sn = (a * qn - b * qe) / det;
    return;
  }
  const double hd = 0.5 * (a - c);
  const double lam = half + sqrt(hd * hd + b * b);
  double ve = lam - c, vn = b;                // (H - c I) column; its sibling (b, lam - a) where this one vanishes
  const double we = b, wn = lam - a;
  if (we * we + wn * wn > ve * ve + vn * vn) ve = we, vn = wn;
  const double n2 = ve * ve + vn * vn;
  if (!(n2 > 0.0) || !(lam > 0.0)) {
    *se = *sn = 0.0;
    return;
  }
  const double proj = (ve * qe + vn * qn) / (n2 * lam);
  *se = ve * proj;
  *sn = vn * proj;
}

// One wave per baseline row, four rows per block (row_walk.hpp).  z_r, z_i hold the reference on entry and z0 on exit.
template <typename T>
__global__ __launch_bounds__(256) void degen_rows_kernel(const T* __restrict__ model_r, const T* __restrict__ model_i, T* __restrict__ z_r,
                                                          T* __restrict__ z_i, const T* __restrict__ wgts, const int2* __restrict__ bl_ant, int nbls,
                                                          int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {
    const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
    const vec_t sr = R.load(z_r, f), si = R.load(z_i, f);
    const vec_t w = R.load(wgts, f);
    vec_t o_r, o_i;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const bool live = f + c < nfreqs && w[c] > (T)0;
      const T cr = mr[c] * sr[c] + mi[c] * si[c];  // conj(m) s
      const T ci = mr[c] * si[c] - mi[c] * sr[c];
      o_r[c] = live ? w[c] * cr : (T)0;
      o_i[c] = live ? w[c] * ci : (T)0;
    }
    R.store(z_r, f, o_r);
    R.store(z_i, f, o_i);
  }
}

// block = (segment, 256 channels); a thread owns one channel and walks the segment's rows in ascending order: a wave reads 64 adjacent
// channels of a row per plane, and the row index, d_b and the slice are block-uniform.  FIRST (Phi = 0: no rotation) also gives Q, H
// and the count.  part: [sums][nseg][fpad].
template <typename T, bool FIRST>
__global__ __launch_bounds__(256) void degen_sum_kernel(const T* __restrict__ z_r, const T* __restrict__ z_i, const T* __restrict__ model_r,
                                                         const T* __restrict__ model_i, const T* __restrict__ wgts, const int* __restrict__ ent,
                                                         const DgSeg* __restrict__ segs, const double2* __restrict__ dvec,
                                                         const double* __restrict__ st, int nsl, int nfreqs, int fpad, int nseg,
                                                         double* __restrict__ part) {
#pragma clang fp contract(off)
  const int f = blockIdx.y * 256 + threadIdx.x;
  if (f >= nfreqs) return;
  const DgSeg sg = segs[blockIdx.x];
  const long long plane = (long long)nsl * fpad;
  const long long sf = (long long)sg.slice * fpad + f;
  const double pe = FIRST ? 0.0 : st[DG_PE * plane + sf], pn = FIRST ? 0.0 : st[DG_PN * plane + sf];
  double qe = 0, qn = 0, sre = 0, Q = 0, hee = 0, hen = 0, hnn = 0, cnt = 0;
#pragma unroll 4
  for (int e = sg.e0; e < sg.e1; ++e) {
    const int b = ent[e];
    const double2 d = dvec[b];
    const long long o = (long long)b * fpad + f;
    const double zr = (double)z_r[o], zi = (double)z_i[o];
    double re = zr, im = zi;
    if (!FIRST) {
      double s, c;
      sincos(pe * d.x + pn * d.y, &s, &c);
      re = zr * c + zi * s;  // z0 e^{-i Phi.d}
      im = zi * c - zr * s;
    }
    qe += im * d.x;
    qn += im * d.y;
    sre += re;
    if (FIRST) {
      const double a = sqrt(zr * zr + zi * zi);
      hee += a * d.x * d.x;
      hen += a * d.x * d.y;
      hnn += a * d.y * d.y;
      const T w = wgts[o], mr = model_r[o], mi = model_i[o];
      const bool live = w > (T)0;
      const T qw = w * (mr * mr + mi * mi);
      Q += live ? (double)qw : 0.0;
      cnt += live ? 1.0 : 0.0;
    }
  }
  const long long sp = (long long)nseg * fpad, po = (long long)blockIdx.x * fpad + f;
  part[0 * sp + po] = qe;
  part[1 * sp + po] = qn;
  part[2 * sp + po] = sre;
  if (FIRST) {
    part[3 * sp + po] = Q;
    part[4 * sp + po] = hee;
    part[5 * sp + po] = hen;
    part[6 * sp + po] = hnn;
    part[7 * sp + po] = cnt;
  }
}

// A channel is empty where Q, tr H or (at the end) the amplitude vanish: it keeps the identity.
__device__ __forceinline__ bool dg_live(double Q, double hee, double hnn) { return Q > 0.0 && hee + hnn > 0.0; }

// stage 0, block = (64 channels x kDgParts waves, slice): the slice's n segments are cut into kDgParts runs of ceil(n / kDgParts); wave y adds
// run y in ascending order, wave 0 then adds the runs in ascending order (an order the slice's own segment count decides) into the state;
// CAL_DEGEN_CHANNEL then takes the channel's step, or with `last` sets eta.  stage 1 (CAL_DEGEN_BAND), block = slice: thread 0 sums the channels in ascending
// order (q_0 = sum r_f q, H_0 = sum r_f^2 H; with `last` sum Re z / sum Q), every thread then sets Phi(f) = r_f Phi_0 for its channels.
// seg_ptr: [nsl + 1] first segment of every slice; ratio: [fpad] nu_f / nu_ref; maxd: [nsl] the longest |d_b| of the slice.
__global__ __launch_bounds__(64 * kDgParts) void degen_solve_kernel(const double* __restrict__ part, const int* __restrict__ seg_ptr, const double* __restrict__ ratio,
                                                           const double* __restrict__ maxd, int band, int stage, int first, int last, int nsl,
                                                           int nfreqs, int fpad, int nseg, double* __restrict__ st) {
#pragma clang fp contract(off)
  const long long plane = (long long)nsl * fpad;
  if (stage == 0) {
    __shared__ double runs[kDgParts][kDgFirstSums][64];
    const int t = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x, run = threadIdx.y;
    const bool on = f < nfreqs;
    const long long sf = (long long)t * fpad + f, sp = (long long)nseg * fpad;
    const int nk = first ? kDgFirstSums : kDgIterSums;
    const int s0 = seg_ptr[t], s1 = seg_ptr[t + 1], per = (s1 - s0 + kDgParts - 1) / kDgParts;
    const int a0 = s0 + run * per, a1 = a0 + per < s1 ? a0 + per : s1;
    double acc[kDgFirstSums];
#pragma unroll
    for (int k = 0; k < kDgFirstSums; ++k) acc[k] = 0.0;
    for (int sgi = a0; sgi < a1 && on; ++sgi) {
#pragma unroll
      for (int k = 0; k < kDgFirstSums; ++k)
        if (k < nk) acc[k] += part[k * sp + (long long)sgi * fpad + f];
    }
#pragma unroll
    for (int k = 0; k < kDgFirstSums; ++k) runs[run][k][threadIdx.x] = acc[k];
    __syncthreads();
    if (run != 0 || !on) return;
#pragma unroll
    for (int k = 0; k < kDgFirstSums; ++k) {
      double v = runs[0][k][threadIdx.x];
      for (int r = 1; r < kDgParts; ++r) v += runs[r][k][threadIdx.x];
      acc[k] = v;
    }
    st[DG_QE * plane + sf] = acc[0];
    st[DG_QN * plane + sf] = acc[1];
    st[DG_SRE * plane + sf] = acc[2];
    if (first) {
      st[DG_Q * plane + sf] = acc[3];
      st[DG_HEE * plane + sf] = acc[4];
      st[DG_HEN * plane + sf] = acc[5];
      st[DG_HNN * plane + sf] = acc[6];
      st[DG_CNT * plane + sf] = acc[7];
    }
    if (band) return;
    const double Q = st[DG_Q * plane + sf], hee = st[DG_HEE * plane + sf], hen = st[DG_HEN * plane + sf], hnn = st[DG_HNN * plane + sf];
    const bool live = dg_live(Q, hee, hnn);
    if (!last) {
      double se = 0.0, sn = 0.0;
      if (live) dg_step2(hee, hen, hnn, acc[0], acc[1], &se, &sn);
      st[DG_PE * plane + sf] += se;
      st[DG_PN * plane + sf] += sn;
      st[DG_STEP * plane + sf] = sqrt(se * se + sn * sn) * maxd[t];
      return;
    }
    const bool ok = live && acc[2] > 0.0;
    const double amp2 = ok ? acc[2] / Q : 1.0;
    st[DG_AMP2 * plane + sf] = amp2;
    st[DG_ETA * plane + sf] = ok ? 0.5 * log(amp2) : 0.0;
    if (!ok) st[DG_PE * plane + sf] = st[DG_PN * plane + sf] = st[DG_STEP * plane + sf] = st[DG_CNT * plane + sf] = 0.0;
    return;
  }
  // ---- stage 1: one sky shift and one amplitude per slice
  __shared__ double sh[3];
  const int t = blockIdx.x;
  double* __restrict__ phi0 = st + kDgPlanes * plane + 2 * t;
  if (threadIdx.x == 0) {
    double qe = 0, qn = 0, hee = 0, hen = 0, hnn = 0, sre = 0, Q = 0;
    for (int f = 0; f < nfreqs; ++f) {
      const long long sf = (long long)t * fpad + f;
      const double Qf = st[DG_Q * plane + sf], a = st[DG_HEE * plane + sf], b = st[DG_HEN * plane + sf], c = st[DG_HNN * plane + sf];
      if (!dg_live(Qf, a, c)) continue;
      const double r = ratio[f];
      qe += r * st[DG_QE * plane + sf];
      qn += r * st[DG_QN * plane + sf];
      hee += r * r * a;
      hen += r * r * b;
      hnn += r * r * c;
      sre += st[DG_SRE * plane + sf];
      Q += Qf;
    }
    const bool live = dg_live(Q, hee, hnn);
    double se = 0.0, sn = 0.0;
    if (!last) {
      if (live) dg_step2(hee, hen, hnn, qe, qn, &se, &sn);
      phi0[0] += se;
      phi0[1] += sn;
      sh[2] = 1.0;
    } else {
      const bool ok = live && sre > 0.0;
      sh[2] = ok ? sre / Q : 0.0;  // 0: the band is empty
    }
    sh[0] = se;
    sh[1] = sn;
  }
  __syncthreads();
  const double pe = phi0[0], pn = phi0[1], step = sqrt(sh[0] * sh[0] + sh[1] * sh[1]) * maxd[t], amp2 = sh[2];
  for (int f = threadIdx.x; f < nfreqs; f += 256) {
    const long long sf = (long long)t * fpad + f;
    const bool live = dg_live(st[DG_Q * plane + sf], st[DG_HEE * plane + sf], st[DG_HNN * plane + sf]) && amp2 > 0.0;
    const double r = ratio[f];
    if (!last) {
      st[DG_PE * plane + sf] = live ? r * pe : 0.0;
      st[DG_PN * plane + sf] = live ? r * pn : 0.0;
      st[DG_STEP * plane + sf] = live ? fabs(r) * step : 0.0;
      continue;
    }
    st[DG_AMP2 * plane + sf] = live ? amp2 : 1.0;
    st[DG_ETA * plane + sf] = live ? 0.5 * log(amp2) : 0.0;
    if (!live) st[DG_PE * plane + sf] = st[DG_PN * plane + sf] = st[DG_STEP * plane + sf] = st[DG_CNT * plane + sf] = 0.0;
  }
}

// block = (64 channels, slice); a thread owns one channel and walks the slice's antennas in ascending order.  An antenna counts when
// one of its cross-correlation rows has w > 0 at the channel (ant_ptr / ant_ent: the antennas' row lists, other antenna in .y).
// antpos: [na] (east, north) of a slice's antennas.
template <typename T>
__global__ __launch_bounds__(64) void degen_phase_kernel(const vec2_t<T>* __restrict__ gains, const vec2_t<T>* __restrict__ gref, const T* __restrict__ wgts,
                                                          const int* __restrict__ ant_ptr, const int2* __restrict__ ant_ent,
                                                          const double2* __restrict__ antpos, int nsl, int na, int nfreqs, int fpad,
                                                          double* __restrict__ st) {
#pragma clang fp contract(off)
  const int t = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x;
  if (f >= nfreqs) return;
  const long long plane = (long long)nsl * fpad, sf = (long long)t * fpad + f;
  if (!(st[DG_CNT * plane + sf] > 0.0)) return;  // empty: psi stays 0
  const double pe = st[DG_PE * plane + sf], pn = st[DG_PN * plane + sf];
  double ar = 0, ai = 0;
  for (int k = 0; k < na; ++k) {
    const int a = t * na + k;
    bool live = false;
    for (int e = ant_ptr[a]; e < ant_ptr[a + 1] && !live; ++e) {
      const int2 en = ant_ent[e];
      live = en.y != a && wgts[(long long)(en.x >> 1) * fpad + f] > (T)0;
    }
    if (!live) continue;
    const vec2_t<T> g = gains[(long long)a * fpad + f], h = gref[(long long)a * fpad + f];
    const double2 r = antpos[k];
    double s, c;
    sincos(pe * r.x + pn * r.y, &s, &c);
    const double gr = (double)g.x, gi = (double)g.y, hr = (double)h.x, hi = (double)h.y;
    const double ur = gr * c + gi * s, ui = gi * c - gr * s;  // g e^{-i Phi.r}
    ar += ur * hr + ui * hi;                                  // ... conj(gref)
    ai += ui * hr - ur * hi;
  }
  st[DG_PSI * plane + sf] = atan2(ai, ar);
}

// thread = (antenna row, channel): g' = g e^{-eta} e^{-i (Phi.r_a + psi)} in double, rounded once; zeros in [nfreqs, fpad).
template <typename T>
__global__ __launch_bounds__(256) void degen_apply_gains_kernel(const vec2_t<T>* __restrict__ gains, const double2* __restrict__ antpos,
                                                                 const double* __restrict__ st, int nsl, int na, int nants, int nfreqs, int fpad,
                                                                 vec2_t<T>* __restrict__ out) {
#pragma clang fp contract(off)
  const long long n = (long long)nants * fpad, plane = (long long)nsl * fpad;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int a = (int)(i / fpad), f = (int)(i - (long long)a * fpad);
    vec2_t<T> o;
    o.x = o.y = (T)0;
    if (f < nfreqs) {
      const long long sf = (long long)(a / na) * fpad + f;
      const double2 r = antpos[a % na];
      const double fac = 1.0 / sqrt(st[DG_AMP2 * plane + sf]);
      double s, c;
      sincos(st[DG_PE * plane + sf] * r.x + st[DG_PN * plane + sf] * r.y + st[DG_PSI * plane + sf], &s, &c);
      const vec2_t<T> g = gains[i];
      const double gr = (double)g.x, gi = (double)g.y;
      o.x = (T)(fac * (gr * c + gi * s));
      o.y = (T)(fac * (gi * c - gr * s));
    }
    out[i] = o;
  }
}

// One wave per baseline row (row_walk.hpp): m' = m e^{2 eta} e^{i Phi.d_b} in double, rounded once, in place; zeros in [nfreqs, fpad).
template <typename T>
__global__ __launch_bounds__(256) void degen_apply_rows_kernel(T* __restrict__ model_r, T* __restrict__ model_i, const int2* __restrict__ bl_ant,
                                                                const double2* __restrict__ dvec, const double* __restrict__ st, int nsl, int na,
                                                                int nbls, int nfreqs, int fpad) {
#pragma clang fp contract(off)
  constexpr int V = RowWalk<T>::V;
  typedef typename RowWalk<T>::vec_t vec_t;
  RowWalk<T> R;
  if (!R.begin(bl_ant, nbls, fpad)) return;
  const double2 d = dvec[R.b];
  const long long plane = (long long)nsl * fpad, s0 = (long long)(R.ant.x / na) * fpad;
  for (int f = R.lane * V; f < fpad; f += 64 * V) {
    const vec_t mr = R.load(model_r, f), mi = R.load(model_i, f);
    vec_t o_r, o_i;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      o_r[c] = o_i[c] = (T)0;
      if (f + c >= nfreqs) continue;
      const long long sf = s0 + f + c;
      const double amp2 = st[DG_AMP2 * plane + sf];
      double s, co;
      sincos(st[DG_PE * plane + sf] * d.x + st[DG_PN * plane + sf] * d.y, &s, &co);
      const double xr = (double)mr[c], xi = (double)mi[c];
      o_r[c] = (T)(amp2 * (xr * co - xi * s));
      o_i[c] = (T)(amp2 * (xi * co + xr * s));
    }
    R.store(model_r, f, o_r);
    R.store(model_i, f, o_i);
  }
}

}  // namespace calk
