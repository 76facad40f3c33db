// fit_kernels.hpp -- hand-written CDNA4 (gfx950) kernels of the gain + foreground fitter.
//
// What they replace (all /root/reference/calamity/calibration.py):
//   fused_basis_kernel : fg_model :1587-1590 (A c), data_model :1593-1605 (gather gains, G = g_i conj(g_j), m = G v),
//                        mse :1608-1609 (weighted chi^2), the "sum" regulariser sums :1648-1649, and the
//                        reverse-mode adjoints tf.GradientTape produces for them (:664-666): A^T gbar_v and gbar_G.
//   gain_grad_kernel   : the scatter-add that is the gradient of tf.gather (:1594-1597) -- done as a sorted
//                        per-antenna segmented reduction, deterministic, no float atomics.
//   adam2_kernel       : opt.apply_gradients (:667) for tf.optimizers.Adam / Adamax (Keras semantics), applied to
//                        the re and im variables independently (:596-603).
//   finalize_kernel    : loss.numpy(), the use_min bookkeeping and the tolerance test of the python loop (:699-717),
//                        kept on the device so a step needs no host synchronisation.
//
// Design (MI355X): the basis is stored tile-major in HBM -- per baseline [channel block][vector][FB channels] -- so one
// workgroup streams each (baseline, channel block) tile exactly once with 16-byte coalesced loads and runs forward AND
// adjoint out of the registers the tile was loaded into (process_item); LDS carries only per-channel vectors.  Several
// workgroups per CU keep > 100 KB per CU in flight.  Fitting groups of several baselines go through process_group_item,
// which shares one tile load / forward / adjoint among the baselines of a redundant run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace calk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
#ifndef CAL_TILE_LOADS
#define CAL_TILE_LOADS 7
#endif
constexpr int kTileBytes = CAL_TILE_LOADS * 4096;  // loads per thread x (256 threads x 16 B)
constexpr int kMaxLoads = kTileBytes / (kThreads * 16);

template <typename T> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };
template <typename T> using vec2_t = typename Vec2<T>::type;

// device-resident loop state: everything the python loop of calibration.py:681-738 keeps on the host
struct DevState {
  double loss;        // loss of the current step (pre-update)
  double prev_loss;   // previous RECORDED loss
  double min_loss;    // use_min bookkeeping, starts at 9e99 (:574)
  double s_r, s_i;    // sum w m (regulariser)
  double alpha_r, alpha_i;  // 2 (S - P)
  double prior_r, prior_i;
  double tol;
  double lr, beta1, beta2, eps;
  double lr_t, lr_u, bc1;   // bias-corrected step sizes of the current step (Adam, Adamax)
  double b1t, b2t;          // beta1^t, beta2^t as running products (a pow() per step and per block of the update kernel is
                            // what the tail of a small step consists of)
  long long t;        // optimizer iterations
  int n_recorded;     // recorded losses written so far in this run
  int n_recorded_total;  // recorded steps since the loop began ("step" of :699)
  int done;           // loop has ended: every kernel of later steps returns at once
  int done_after;     // this step decided to stop: later steps see done
  int improved;       // use_min: this step's loss is the new minimum
  int record;
  int use_min;
  int reg;
  int nonfinite;
  int nupdates;
  int f32;            // the fit runs in float32: loop decisions compare float32 losses, as loss.numpy() of a float32 fit does (:701, :712)
  int opt;            // cal_optimizer (OPTIMIZERS, :17-27)
  int nesterov;       // SGD
  double momentum, rho;      // SGD / RMSprop momentum; RMSprop / Adadelta decay
  double nadam_sched;        // Nadam: running product of its momentum schedule (Keras' _m_cache), 1 before the first update
  double ftrl[4];            // Ftrl: learning_rate_power, l1, l2 + beta / (2 lr), l2_shrinkage
  double k[6];               // the current step's update coefficients, per optimizer: see optimizer_step
};
enum { OPT_ADAM = 0, OPT_ADAMAX = 1, OPT_SGD = 2, OPT_RMSPROP = 3, OPT_ADAGRAD = 4, OPT_NADAM = 5, OPT_ADADELTA = 6, OPT_FTRL = 7, OPT_LAMB = 8 };

// Time slices (cal_problem_desc::nslices): one solver may hold several independent fits -- the (polarization, time) slices the
// reference fits one after another (calibration.py:1160-1167) -- each with its own gains (antennas [t na_slice, (t + 1) na_slice)),
// coefficients (a contiguous run of the flat planes), loss, regulariser sums and loop state.  DevState is an array with one entry
// per slice; every kernel looks up the state of the slice its work belongs to, so a slice stops (tolerance, :712-717), keeps its
// minimum (:702-710) and records its losses (:701) on its own.
struct SliceMap {
  const int* coff;      // [nslices + 1] first coefficient of every slice (offsets into one plane)
  const int* part_ptr;  // [nslices + 1] the loss partials of slice t are entries part_ptr[t] .. part_ptr[t + 1] of part_idx
  const int* part_idx;  // [nparts] indices into `part` grouped by slice; nullptr with one slice (identity)
  int nslices;
  int na_slice;         // antennas per slice
};
__device__ __forceinline__ int slice_of_coef(const SliceMap& M, int n) {  // largest t with coff[t] <= n
  int lo = 0, hi = M.nslices - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (M.coff[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct Item {        // one workgroup's share of a fitting group
  int bl0;           // first baseline of the GROUP
  int tile0, tile1;  // linear tile range inside the group: tile = (bl - bl0) * ntpb + channel_block
  int nvec;
  int coff;          // offset of the group's coefficients in the flat coefficient planes
  int goff;          // offset of this item's partial coefficient gradient
  int fb_log2;       // log2 of the channel-block width of this group's tiles
  int role_n;        // baselines that read the SAME tiles (cal_problem_desc::bl_alias): 0 = an ordinary item; (n << 2) | 1 = head of a
                     // set of n such baselines, processed by fused_multi_kernel; 2 = member covered by a head.  Heads and members
                     // stay complete single-baseline items: the passes without a multi form (model, initial coefficients, the
                     // two-adjoint-set regulariser) run them one by one
  // single-baseline groups: tile offset and antenna pair of the baseline the item starts with (bl_tile / bl_ant of it), so
  // that the item's first tile loads do not wait for a lookup of their own
  long long tile_first;
  int2 ant_first;
  int member0;       // head: its first entry in FusedArgs::members
  int slice;         // the time slice (cal_problem_desc::nslices) the item's group belongs to: which DevState governs it
};

struct Member {      // one baseline of a set that shares tiles
  int bl;            // row of its samples
  int coff;          // its group's coefficients
  int goff;          // where its coefficient gradient goes (its own item's slot)
  int ant0, ant1;
  int slice;         // its time slice
  int item;          // its own item: where its loss partial goes (FusedArgs::part)
  int pad;
};
template <typename T> struct MultiCfg { static constexpr int nb_max = sizeof(T) == 4 ? 8 : 4; };  // baselines per multi item (gradient accumulators live in registers)

template <typename T>
struct FusedArgs {
  const T* tiles;            // all basis tiles
  const long long* bl_tile;  // [nbls] element offset of the baseline's first tile
  const int2* bl_ant;        // [nbls] (ant0, ant1)
  const T* data_r;           // [nbls][fpad]
  const T* data_i;
  const T* wgts;
  const vec2_t<T>* gains;    // [nants][fpad] (re, im)
  const T* c_r;              // [ncoef]
  const T* c_i;
  const Item* items;
  vec2_t<T>* q0;             // [nbls][fpad] gbar_G for e0
  vec2_t<T>* q1;             // [nbls][fpad] gbar_G for the w part (regulariser) or nullptr
  T* gcp0_r; T* gcp0_i;      // partial coefficient gradients
  T* gcp1_r; T* gcp1_i;
  double* part;              // [nitems][4]: loss, s_r, s_i, unused
  T* model_r; T* model_i;    // MODE_MODEL output [nbls][fpad]
  const DevState* state;     // [nslices] loop state of every time slice (the current half of the double buffer)
  int nslices;
  int fpad;
  int nbls;                  // q0 / q1 have nbls + 1 rows; row nbls stays zero
  int stream_once;           // CAL_LAYOUT_STREAM: every tile is read once per pass
  const int2* runs;          // group kernel: [nruns] (first baseline, one past the last) of baselines that share a row block
  int item_base;             // index of this launch's first item in `items` / `part`
  const Member* members;     // multi kernel: the baselines of every head item
  const int* heads;          // multi kernel: [grid] item index of each head
  int nfreqs;                // channels of the band (folded tiles: channel f and its mirror nfreqs - 1 - f travel together)
};

enum { MODE_LOSS = 0, MODE_GRAD = 1, MODE_MODEL = 2, MODE_INIT = 3 };  // INIT: c = A^T (src * [w != 0]), calibration.py:875-902

template <typename T, int FB>
struct TileCfg {
  static constexpr int VEC = 16 / (int)sizeof(T);      // reals per 16-byte load
  static constexpr int MAXK = kTileBytes / (int)sizeof(T) / FB;  // basis vectors (rows) a tile can hold
  static constexpr int LPR = FB / VEC;                 // lanes that hold one row of the tile
  static constexpr int NS = kThreads / LPR;            // rows covered by one 256-thread load = MAXK / kMaxLoads
  static constexpr int QT = 1024 / FB;                 // tiles of gbar_G the LDS buffer holds (1024 channels)
  // fold: the even- and the odd-vector partials stay apart and gbar_v covers the tile's mirror channels too
  static constexpr size_t lds_bytes(bool fold = false) {
    return ((fold ? 4 : 2) * (size_t)kWaves * FB + (fold ? 4 : 2) * (size_t)FB + MAXK) * 2 * sizeof(T)  // forward partials (two parities), gbar_v, c
           + 64;
  }
  // MODE_GRAD only: gbar_G rows (and the regulariser's second set) waiting for the flush, and their row offsets
  static constexpr size_t q_lds_bytes(bool reg) { return (reg ? 2 : 1) * (size_t)1024 * 2 * sizeof(T) + QT * sizeof(long long); }
};

// acc (re, im) += a[u] * b (re, im) for the four reals a[0..3] of one 16-byte load: v_pk_fma_f32 broadcasts either half
// of a 64-bit operand through op_sel, so no register shuffling is needed.  (hipcc matches only part of these broadcasts
// and pads the rest with v_mov: 64 moves beside 62 packed FMAs per tile before this was written out.)
typedef float pair_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pk_fma_lo(pair_t& acc, pair_t a, pair_t b) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void pk_fma_hi(pair_t& acc, pair_t a, pair_t b) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(a), "v"(b));
}
// acc[0..3] += a[0..3] (x) b : four (re, im) accumulators, one per real of the load
__device__ __forceinline__ void fma_rows(float2* acc, const float __attribute__((ext_vector_type(4))) a, const float2 b) {
  const pair_t a01 = {a[0], a[1]}, a23 = {a[2], a[3]}, bb = {b.x, b.y};
  pair_t* p = reinterpret_cast<pair_t*>(acc);
  pk_fma_lo(p[0], a01, bb);
  pk_fma_hi(p[1], a01, bb);
  pk_fma_lo(p[2], a23, bb);
  pk_fma_hi(p[3], a23, bb);
}
// acc += sum_u a[u] * b[u] : one (re, im) accumulator
__device__ __forceinline__ void fma_cols(float2& acc, const float __attribute__((ext_vector_type(4))) a, const float2* b) {
  const pair_t a01 = {a[0], a[1]}, a23 = {a[2], a[3]};
  pair_t& p = reinterpret_cast<pair_t&>(acc);
  pk_fma_lo(p, a01, pair_t{b[0].x, b[0].y});
  pk_fma_hi(p, a01, pair_t{b[1].x, b[1].y});
  pk_fma_lo(p, a23, pair_t{b[2].x, b[2].y});
  pk_fma_hi(p, a23, pair_t{b[3].x, b[3].y});
}
__device__ __forceinline__ void fma_rows(double2* acc, const double __attribute__((ext_vector_type(2))) a, const double2 b) {
  acc[0].x += a[0] * b.x;
  acc[0].y += a[0] * b.y;
  acc[1].x += a[1] * b.x;
  acc[1].y += a[1] * b.y;
}
__device__ __forceinline__ void fma_cols(double2& acc, const double __attribute__((ext_vector_type(2))) a, const double2* b) {
  acc.x += a[0] * b[0].x + a[1] * b[1].x;
  acc.y += a[0] * b[0].y + a[1] * b[1].y;
}

// Fused multiply-add spelled out.  Code that two different kernels must evaluate to the SAME bits (the launch forms of a step:
// gain_grad_kernel / step_tail_kernel, combine_* / step_tail_kernel, every update kernel) cannot leave a * b + c to the
// compiler, which contracts it or not depending on the surrounding code: it uses fma_() where a fused operation is wanted and
// `#pragma clang fp contract(off)` where it is not.
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// x + (x of lane ^ SFT) without the LDS crossbar: ds_bpermute, which __shfl_xor compiles to, occupies the CU's LDS pipe,
// and the forward product of every tile ends in such a reduction over the lanes that hold the other rows (2116 ds_bpermute
// in the multi-slice kernel).  gfx950 swaps lane halves / rows of 16 in the vector ALU (v_permlane32_swap, v_permlane16_swap:
// with both operands x, result 0 carries the lower partner's x and result 1 the upper partner's on BOTH lanes); a rotation by
// 8 inside a row of 16 is a DPP modifier.  Smaller strides (tiles of 16 or 8 channels: blocks of more than 224 vectors) keep
// the shuffle.  Same pairs, same single addition: the sums are bit for bit those of the shuffle form.
__device__ __forceinline__ float pair_sum32(float x) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const u2 r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
  const unsigned a = r[0], b = r[1];
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float pair_sum16(float x) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const u2 r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
  const unsigned a = r[0], b = r[1];
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float pair_sum8(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xf, 0xf, true);  // row_ror:8
  return x + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ double pair_sum32(double x) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
  const u2 lo = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  const u2 hi = __builtin_amdgcn_permlane32_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
  const unsigned l0 = lo[0], l1 = lo[1], h0 = hi[0], h1 = hi[1];
  return __builtin_bit_cast(double, ((unsigned long long)h0 << 32) | l0) + __builtin_bit_cast(double, ((unsigned long long)h1 << 32) | l1);
}
__device__ __forceinline__ double pair_sum16(double x) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
  const u2 lo = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  const u2 hi = __builtin_amdgcn_permlane16_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
  const unsigned l0 = lo[0], l1 = lo[1], h0 = hi[0], h1 = hi[1];
  return __builtin_bit_cast(double, ((unsigned long long)h0 << 32) | l0) + __builtin_bit_cast(double, ((unsigned long long)h1 << 32) | l1);
}
__device__ __forceinline__ double pair_sum8(double x) {
  const long long b = __builtin_bit_cast(long long, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x128, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x128, 0xf, 0xf, true);
  return x + __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
// sum over the 64 / LPR lanes {lane ^ k LPR}: the rows of a tile held by the other lanes of the wave (ascending strides)
// SPLIT: without the stride-LPR stage, the one that adds rows of the other parity: lanes [0, LPR) end up with the sum over
// the wave's even rows, lanes [LPR, 2 LPR) with the sum over its odd rows (folded tiles)
template <int LPR, bool SPLIT = false, typename T> __device__ __forceinline__ T sum_row_lanes(T x) {
  if constexpr (LPR <= 1 && !(SPLIT && LPR == 1)) x += __shfl_xor(x, 1, 64);
  if constexpr (LPR <= 2 && !(SPLIT && LPR == 2)) x += __shfl_xor(x, 2, 64);
  if constexpr (LPR <= 4 && !(SPLIT && LPR == 4)) x += __shfl_xor(x, 4, 64);
  if constexpr (LPR <= 8 && !(SPLIT && LPR == 8)) x = pair_sum8(x);
  if constexpr (LPR <= 16 && !(SPLIT && LPR == 16)) x = pair_sum16(x);
  if constexpr (LPR <= 32 && !(SPLIT && LPR == 32)) x = pair_sum32(x);
  return x;
}

template <typename T> __device__ __forceinline__ T ldsum(T v) {
  // full-wave butterfly sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One item: stream its tiles once; forward and adjoint run out of the registers the tile was loaded into.
//
// A tile is [nvec][FB] reals, row-major.  The 16-byte load l of thread tid covers row k = l * NS + tid / LPR, channels
// f0 = (tid % LPR) * VEC ... f0 + VEC - 1, so every thread owns the same kMaxLoads rows and VEC channels in every tile
// of the item.  That makes both products register-resident:
//   forward  v[f]  = sum_k A[k][f] c[k]      : per thread a partial over its rows (coefficients of those rows stay
//                                              in registers for the whole item), summed over the threads that share
//                                              the channels: shuffles inside the wave, 4 x FB pairs through LDS
//   adjoint  gc[k] = sum_f A[k][f] gbar_v[f] : per thread a partial over its channels, ACCUMULATED over all tiles of
//                                              the item in registers and summed over the LPR lanes of a row once,
//                                              at the end of the item
// LDS carries only per-channel vectors (about 17 KB of traffic per 28 KB tile); the tile itself never enters it.
// L: 16-byte loads per thread and tile the body is unrolled for (rows l NS + ks, l < L): kMaxLoads covers every tile; problems whose
// blocks all fit two loads (the tutorial's: at most 2 NS vectors) run an instance with L = 2 -- a fraction of the registers, twice
// the workgroups per CU, no loads and products spent on rows past nvec
//
// FOLD: the basis is mirror-symmetric about the band centre, A[F-1-f][k] = (-1)^k A[f][k] (discrete prolate spheroidal
// sequences centred on zero delay), and only its channels [0, F/2) are in HBM.  A tile then serves its FB channels AND their
// FB mirror channels:
//   forward  E[f] = sum over even k, O[f] = sum over odd k;   v[f] = E[f] + O[f],   v[F-1-f] = E[f] - O[f]
//   adjoint  gc[k] = sum_{f < F/2} A[k][f] (gbar_v[f] + (-1)^k gbar_v[F-1-f])
// NS is even for every FB, so all rows l NS + ks of a thread have the parity of ks: its forward partial is purely an E or
// purely an O partial, and its adjoint needs one of the two combinations only.  The products per loaded byte stay the same;
// the bytes halve.  The per-channel stage runs on 2 FB threads (the second FB take the mirror block, in that block's own
// channel order); tiles are counted in folded tiles: tile j = channel blocks j and F / FB - 1 - j.
template <typename T, int FB, int MODE, bool REG, int L = kMaxLoads, bool FOLD = false>
__device__ __forceinline__ void process_item(const FusedArgs<T>& A, const Item it, unsigned char* smem, int item_idx, const DevState* st_own) {
  using C = TileCfg<T, FB>;
  using T2 = vec2_t<T>;
  constexpr int VEC = C::VEC;
  constexpr int LPR = C::LPR;
  constexpr int NS = C::NS;
  constexpr bool FWD = (MODE != MODE_INIT);
  constexpr bool BWD = (MODE == MODE_GRAD || MODE == MODE_INIT);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fq = tid % LPR;
  const int ks = tid / LPR;
  const int f0 = fq * VEC;
  const int nvec = it.nvec;
  constexpr int NP = FOLD ? 2 : 1;          // row parities kept apart in the forward partials; channel blocks per tile
  constexpr int CH = NP * FB;               // channels of the per-channel stage
  const int ntpb = FOLD ? A.nfreqs / (2 * FB) : A.fpad / FB;
  const int tile_elems = nvec * FB;

  T2* s_pv = reinterpret_cast<T2*>(smem);   // [2][kWaves][NP][FB] forward partials of the four waves, by tile parity
  T2* s_gv = s_pv + 2 * kWaves * CH;        // [2][NP][FB]: gbar_v of e0, of the w part (regulariser); FOLD: [.][1][i] belongs to the mirror of channel i
  T2* s_c = s_gv + 2 * CH;                  // [MAXK] coefficients of the group
  T2* s_q = s_c + C::MAXK;                  // MODE_GRAD: [REG ? 2 : 1][QT][FB] gbar_G rows waiting for the flush
  long long* s_qo = reinterpret_cast<long long*>(s_q + (REG ? 2 : 1) * C::QT * FB);  // [QT] their offsets in q0 / q1

  typedef T stage_t __attribute__((ext_vector_type(16 / sizeof(T))));

  // coefficients of the group, (re, im) pairs, zero beyond nvec (those rows are not loaded either).  They are read
  // back per tile rather than held in 2 x kMaxLoads registers: registers decide how many workgroups share a CU
  // (several time slices: the stop flags of the item's OWN slice depend on the item record, like the coefficients: requested with
  // them -- one round trip, not two -- and acted on behind them; nothing has been written yet)
  int own_stop = 0;
  if (st_own) own_stop = st_own->done | st_own->done_after;
  if (FWD) {
    for (int k = tid; k < C::MAXK; k += kThreads) {
      T2 c;
      c.x = k < nvec ? A.c_r[it.coff + k] : (T)0;
      c.y = k < nvec ? A.c_i[it.coff + k] : (T)0;
      s_c[k] = c;
    }
    __syncthreads();
  }
  if (own_stop) return;
  // byte offset of this thread's part of load l inside a tile: the same in every tile of the item
  unsigned voff[L];
#pragma unroll
  for (int l = 0; l < L; ++l) voff[l] = (unsigned)((min(l * NS + ks, nvec - 1) * FB + f0) * (int)sizeof(T));
  T2 acc0[L], acc1[L];
#pragma unroll
  for (int l = 0; l < L; ++l) acc0[l].x = acc0[l].y = acc1[l].x = acc1[l].y = 0;
  double loss_acc = 0.0, sr_acc = 0.0, si_acc = 0.0;

  // gbar_G leaves through LDS, 1024 channels at a time: CDNA4 retires a wave's loads and stores in issue order
  // (vmcnt) and a store is acknowledged later than the loads around it, so a store per tile in front of the next
  // tile's loads delays them (measured: 0.4 ms of 4.9 ms on HERA-350).  The flush of a single-baseline item has no
  // load behind it.
  int q_count = 0;
  auto flush_q = [&]() {
    constexpr int kSlotBytes = FB * (int)sizeof(T2);
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    for (int b = tid * 16; b < q_count * kSlotBytes; b += kThreads * 16) {
      const int slot = b / kSlotBytes;
      const int within = b - slot * kSlotBytes;
      const long long o = s_qo[slot];
      *reinterpret_cast<u4*>(reinterpret_cast<char*>(A.q0 + o) + within) =
          *reinterpret_cast<const u4*>(reinterpret_cast<const char*>(s_q) + b);
      if (REG)
        *reinterpret_cast<u4*>(reinterpret_cast<char*>(A.q1 + o) + within) =
            *reinterpret_cast<const u4*>(reinterpret_cast<const char*>(s_q + C::QT * FB) + b);
    }
    q_count = 0;
  };

  // The items of this kernel belong to single-baseline groups: tile offset and antenna pair are those of the item record
  // (wave-uniform, no lookup behind the item's own load).
  const long long t_off = it.tile_first;
  const int2 ant = it.ant_first;

  for (int tau = it.tile0; tau < it.tile1; ++tau) {
    const int blrel = tau / ntpb;
    const int fbk = tau - blrel * ntpb;
    const int bl = it.bl0 + blrel;
    if (MODE == MODE_GRAD && q_count == C::QT) flush_q();       // s_q was last written before the previous barrier (QT is even: a folded tile's two rows fit)


    // ---- issue everything the tile needs: per-channel operands first (threads < FB), then the tile
    T d_r = 0, d_i = 0, w = 0;
    T2 g0, g1;
    g0.x = g0.y = g1.x = g1.y = 0;
    // the per-channel stage (FB threads) moves to the next group of FB threads with every tile, so that over an item
    // all four SIMDs of the CU carry the same share of it
    const int ch = (tid + CH * (tau % (kThreads / CH))) % kThreads;  // this thread's channel in the per-channel stage
    // FOLD: threads [FB, 2 FB) take the mirror block, channels nfreqs - (fbk + 1) FB + cp in that block's own order;
    // cp is the mirror of channel ci = FB - 1 - cp of the tile
    const bool hi = FOLD && ch >= FB;
    const int cp = hi ? ch - FB : ch;
    const int col = hi ? A.nfreqs - (fbk + 1) * FB + cp : fbk * FB + cp;  // channel of the band
    const long long o_ch = (long long)bl * A.fpad + col;
    if (ch < CH) {
      if (MODE != MODE_MODEL) {
        // read once per pass: non-temporal, like the tiles of the streaming layout
        d_r = __builtin_nontemporal_load(A.data_r + o_ch);
        d_i = __builtin_nontemporal_load(A.data_i + o_ch);
        w = __builtin_nontemporal_load(A.wgts + o_ch);
      }
      if (MODE == MODE_LOSS || MODE == MODE_GRAD) {
        g0 = A.gains[(long long)ant.x * A.fpad + col];
        g1 = A.gains[(long long)ant.y * A.fpad + col];
      }
    }
    // Every load is unconditional and unmasked: a lane-masked load next to a zero fill of the other lanes makes the
    // compiler wait for each load before it touches the register again, seven round trips per tile.  Rows past nvec
    // re-read the last row of the tile (cache hits); their coefficients are zero and their adjoint sums are never
    // written.
    const char* src = reinterpret_cast<const char*>(A.tiles + t_off + (long long)fbk * tile_elems);  // uniform
    stage_t stage[L];
    if (A.stream_once) {
      // per-baseline tiles are read exactly once per pass: non-temporal loads keep them from displacing the gains and
      // the other re-used arrays in L2 / Infinity Cache (measured: LOSS pass 4.09 -> 3.8 ms on HERA-350)
#pragma unroll
      for (int l = 0; l < L; ++l) stage[l] = __builtin_nontemporal_load(reinterpret_cast<const stage_t*>(src + voff[l]));
    } else {
#pragma unroll
      for (int l = 0; l < L; ++l) stage[l] = *reinterpret_cast<const stage_t*>(src + voff[l]);
    }

    // ---- forward
    T2* pv_par = s_pv + (tau & 1) * kWaves * CH;
    if (FWD) {
      T2 pv[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u) pv[u].x = pv[u].y = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        fma_rows(pv, stage[l], s_c[l * NS + ks]);
      }
      // rows held by the other lanes of this wave (FOLD: those of this thread's parity; lane / LPR is 0 for the even, 1 for the odd rows)
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        pv[u].x = sum_row_lanes<LPR, FOLD>(pv[u].x);
        pv[u].y = sum_row_lanes<LPR, FOLD>(pv[u].y);
      }
      if (lane < NP * LPR) {
#pragma unroll
        for (int u = 0; u < VEC; ++u) pv_par[wave * CH + (lane / LPR) * FB + f0 + u] = pv[u];
      }
    }
    __syncthreads();

    // ---- per-channel stage: thread = channel ch
    if (ch < CH) {
      const int ci = hi ? FB - 1 - cp : cp;       // the tile's channel this thread's products come from
      const int gslot = (hi ? FB : 0) + ci;       // where its gbar_v goes
      T vr = 0, vi = 0;
      if (FWD) {
        if (FOLD) {
          T orr = 0, oi = 0;
#pragma unroll
          for (int wv = 0; wv < kWaves; ++wv) {
            const T2 e = pv_par[wv * CH + ci];
            const T2 o = pv_par[wv * CH + FB + ci];
            vr += e.x;
            vi += e.y;
            orr += o.x;
            oi += o.y;
          }
          vr = hi ? vr - orr : vr + orr;
          vi = hi ? vi - oi : vi + oi;
        } else {
#pragma unroll
          for (int wv = 0; wv < kWaves; ++wv) {
            const T2 p = pv_par[wv * FB + ch];
            vr += p.x;
            vi += p.y;
          }
        }
      }
      if (MODE == MODE_MODEL) {
        A.model_r[o_ch] = vr;
        A.model_i[o_ch] = vi;
      } else if (MODE == MODE_INIT) {
        // binary weights of calibration.py:875-877: ~np.isclose(w, 0.0) (atol 1e-8)
        const T msk = (fabs(w) <= (T)1e-8) ? (T)0 : (T)1;
        T2 gv;
        gv.x = d_r * msk;
        gv.y = d_i * msk;
        s_gv[gslot] = gv;
      } else {
        // G = g0 conj(g1)   (calibration.py:1598-1601: grgr + gigi, gigr - grgi)
        const T G_r = g0.x * g1.x + g0.y * g1.y;
        const T G_i = g0.y * g1.x - g0.x * g1.y;
        const T m_r = G_r * vr - G_i * vi;
        const T m_i = G_i * vr + G_r * vi;
        const T r_r = d_r - m_r;
        const T r_i = d_i - m_i;
        loss_acc += (double)(w * (r_r * r_r + r_i * r_i));
        if (REG) {
          sr_acc += (double)(w * m_r);
          si_acc += (double)(w * m_i);
        }
        if (MODE == MODE_GRAD) {
          const T e_r = (T)-2 * w * r_r;
          const T e_i = (T)-2 * w * r_i;
          // gbar_v = conj(G) e
          T2 gv;
          gv.x = G_r * e_r + G_i * e_i;
          gv.y = G_r * e_i - G_i * e_r;
          s_gv[gslot] = gv;
          // gbar_G = conj(v) e   (FOLD: the mirror block is a row of its own, in its own channel order)
          const int qs = q_count + (hi ? 1 : 0);
          T2 q;
          q.x = vr * e_r + vi * e_i;
          q.y = vr * e_i - vi * e_r;
          s_q[qs * FB + cp] = q;
          if (cp == 0) s_qo[qs] = o_ch;
          if (REG) {
            // the part of e that multiplies alpha: w (real)
            T2 gw;
            gw.x = G_r * w;
            gw.y = -G_i * w;
            s_gv[CH + gslot] = gw;
            T2 qw;
            qw.x = vr * w;
            qw.y = -vi * w;
            s_q[(C::QT + qs) * FB + cp] = qw;
          }
        }
      }
    }
    if (BWD) {
      __syncthreads();
      // ---- adjoint: this thread's channels of gbar_v against its rows of the tile
      T2 gv0[VEC], gv1[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        gv0[u] = s_gv[f0 + u];
        if (REG) gv1[u] = s_gv[CH + f0 + u];
        if (FOLD) {
          // gbar_v[f] + (-1)^k gbar_v[F-1-f]: every row of this thread has the parity of ks
          const T sg = (ks & 1) ? (T)-1 : (T)1;
          const T2 m0 = s_gv[FB + f0 + u];
          gv0[u].x = fma_(sg, m0.x, gv0[u].x);
          gv0[u].y = fma_(sg, m0.y, gv0[u].y);
          if (REG) {
            const T2 m1 = s_gv[CH + FB + f0 + u];
            gv1[u].x = fma_(sg, m1.x, gv1[u].x);
            gv1[u].y = fma_(sg, m1.y, gv1[u].y);
          }
        }
      }
#pragma unroll
      for (int l = 0; l < L; ++l) {
        fma_cols(acc0[l], stage[l], gv0);
        if (REG) fma_cols(acc1[l], stage[l], gv1);
      }
      if (MODE == MODE_GRAD) q_count += NP;
    }
    // no barrier here: the next tile writes the other parity of s_pv, and s_gv / s_q are rewritten only behind the
    // next tile's first barrier, which no wave reaches before it has finished this tile
  }

  if (MODE == MODE_GRAD) {
    __syncthreads();
    flush_q();
  }
  // ---- item epilogue: loss partials (double), coefficient-gradient partials
  if (MODE == MODE_LOSS || MODE == MODE_GRAD) {
    __syncthreads();
    double* s_red = reinterpret_cast<double*>(s_pv);  // reuse: 3 x kWaves doubles
    const double l = ldsum(loss_acc);
    const double sr = REG ? ldsum(sr_acc) : 0.0;
    const double si = REG ? ldsum(si_acc) : 0.0;
    if (lane == 0) {
      s_red[wave] = l;
      s_red[kWaves + wave] = sr;
      s_red[2 * kWaves + wave] = si;
    }
    __syncthreads();
    if (tid == 0) {
      double a = 0, b = 0, c = 0;
      for (int wv = 0; wv < kWaves; ++wv) {
        a += s_red[wv];
        b += s_red[kWaves + wv];
        c += s_red[2 * kWaves + wv];
      }
      A.part[(size_t)item_idx * 4 + 0] = a;
      A.part[(size_t)item_idx * 4 + 1] = b;
      A.part[(size_t)item_idx * 4 + 2] = c;
    }
  }
  if (BWD) {
    // sum over the LPR lanes that hold the same rows (they are consecutive lanes of one wave); lane fq == 0 writes
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
      for (int sft = 1; sft < LPR; sft <<= 1) {
        acc0[l].x += __shfl_xor(acc0[l].x, sft, 64);
        acc0[l].y += __shfl_xor(acc0[l].y, sft, 64);
        if (REG) {
          acc1[l].x += __shfl_xor(acc1[l].x, sft, 64);
          acc1[l].y += __shfl_xor(acc1[l].y, sft, 64);
        }
      }
      const int k = l * NS + ks;
      if (fq == 0 && k < nvec) {
        A.gcp0_r[it.goff + k] = acc0[l].x;
        A.gcp0_i[it.goff + k] = acc0[l].y;
        if (REG) {
          A.gcp1_r[it.goff + k] = acc1[l].x;
          A.gcp1_i[it.goff + k] = acc1[l].y;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Several single-baseline groups that read the SAME tiles: the same physical baseline in the time slices a rank fits
// together (cal_problem_desc::bl_alias, STREAM layout; the reference loops over times, calibration.py:1160-1167, and SURVEY
// section 8e "Multiple times" asks for A to be read once for all of them).  The tile is loaded ONCE into the registers of
// process_item's layout and serves the forward product, the per-channel stage and the adjoint of every member: per tile one
// load, two barriers and 2 NB products instead of NB loads and 2 NB barriers -- an item of 8 slices moves an eighth of the
// bytes of 8 single items.  Coefficients of all members sit in LDS, their gradient accumulators in registers (NB <= 8 in
// float32, 4 in float64), gbar_G goes straight to HBM (the pass is no longer bound by the tile stream that a store would delay).
template <typename T, int FB>
constexpr size_t multi_lds_bytes() {
  constexpr int NB = MultiCfg<T>::nb_max;
  return ((size_t)NB * TileCfg<T, FB>::MAXK + (size_t)NB * kWaves * FB + (size_t)NB * FB) * 2 * sizeof(T) + NB * sizeof(Member) + 64;
}
// REG: the "sum" regulariser in two passes (see multi_mfma_item): the loss pass also sums S = sum w m per member, the gradient
// pass applies e = -2 w r + alpha w with the alpha of the member's slice and leaves the loss partials of the loss pass in place
template <typename T, int FB, int MODE, bool REG>
__device__ __forceinline__ void process_multi_item(const FusedArgs<T>& A, const Item it, unsigned char* smem, int item_idx) {
  using C = TileCfg<T, FB>;
  using T2 = vec2_t<T>;
  constexpr int VEC = C::VEC;
  constexpr int LPR = C::LPR;
  constexpr int NS = C::NS;
  constexpr int L = kMaxLoads;
  constexpr int NBMAX = MultiCfg<T>::nb_max;
  constexpr int R = (NBMAX * FB + kThreads - 1) / kThreads;  // (member, channel) pairs of the per-channel stage per thread
  constexpr bool GRAD = MODE == MODE_GRAD;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fq = tid % LPR;
  const int ks = tid / LPR;
  const int f0 = fq * VEC;
  const int nvec = it.nvec;
  const int NB = it.role_n >> 2;
  const int ntpb = A.fpad / FB;
  const int tile_elems = nvec * FB;

  T2* s_c = reinterpret_cast<T2*>(smem);            // [NBMAX][MAXK] coefficients of every member
  T2* s_pv = s_c + NBMAX * C::MAXK;                 // [NBMAX][kWaves][FB] forward partials of the four waves
  T2* s_gv = s_pv + NBMAX * kWaves * FB;            // [NBMAX][FB] gbar_v
  Member* s_mem = reinterpret_cast<Member*>(s_gv + NBMAX * FB);
  typedef T stage_t __attribute__((ext_vector_type(16 / sizeof(T))));

  if (tid < NB * (int)(sizeof(Member) / 4)) reinterpret_cast<int*>(s_mem)[tid] = reinterpret_cast<const int*>(A.members + it.member0)[tid];
  __syncthreads();
  for (int n = tid; n < NB * C::MAXK; n += kThreads) {
    const int m = n / C::MAXK, k = n - m * C::MAXK;
    T2 c;
    c.x = k < nvec ? A.c_r[s_mem[m].coff + k] : (T)0;
    c.y = k < nvec ? A.c_i[s_mem[m].coff + k] : (T)0;
    s_c[n] = c;
  }
  unsigned voff[L];
#pragma unroll
  for (int l = 0; l < L; ++l) voff[l] = (unsigned)((min(l * NS + ks, nvec - 1) * FB + f0) * (int)sizeof(T));
  T2 acc[NBMAX][L];
#pragma unroll
  for (int m = 0; m < NBMAX; ++m)
#pragma unroll
    for (int l = 0; l < L; ++l) acc[m][l].x = acc[m][l].y = 0;
  double loss_acc[R];  // per (member, channel) pair of this thread: each member's loss goes to its OWN slot (its time slice's sum)
  double sr_acc[REG && !GRAD ? R : 1], si_acc[REG && !GRAD ? R : 1];
  T al_r[REG && GRAD ? R : 1], al_i[REG && GRAD ? R : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) loss_acc[r] = 0.0;
#pragma unroll
  for (int r = 0; r < (REG && !GRAD ? R : 1); ++r) sr_acc[r] = si_acc[r] = 0.0;
  // this thread's (member, channel) pairs of the per-channel stage: pair p = r * 256 + tid -> member p / FB, channel p % FB
  int pm[R], pch[R];
  unsigned prow[R];    // sample row of the member: bl * fpad (32-bit element offsets: the host checks (nbls + 1) * fpad < 2^31)
  unsigned pg0[R], pg1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = r * kThreads + tid;
    pm[r] = p / FB;
    pch[r] = p % FB;
    const int mm = min(pm[r], NB - 1);  // pairs past the last member are computed on it and discarded
    prow[r] = (unsigned)s_mem[mm].bl * (unsigned)A.fpad + (unsigned)pch[r];
    pg0[r] = (unsigned)s_mem[mm].ant0 * (unsigned)A.fpad + (unsigned)pch[r];
    pg1[r] = (unsigned)s_mem[mm].ant1 * (unsigned)A.fpad + (unsigned)pch[r];
    if (REG && GRAD) {
      al_r[r] = (T)A.state[s_mem[mm].slice].alpha_r;
      al_i[r] = (T)A.state[s_mem[mm].slice].alpha_i;
    }
  }
  __syncthreads();  // s_c complete

  for (int fbk = 0; fbk < ntpb; ++fbk) {
    // ---- issue: the per-channel operands of this thread's pairs, then the tile (once for all members)
    T d_r[R], d_i[R], w[R];
    T2 g0[R], g1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned o = prow[r] + (unsigned)(fbk * FB);
      d_r[r] = __builtin_nontemporal_load(A.data_r + o);
      d_i[r] = __builtin_nontemporal_load(A.data_i + o);
      w[r] = __builtin_nontemporal_load(A.wgts + o);
      g0[r] = A.gains[pg0[r] + (unsigned)(fbk * FB)];
      g1[r] = A.gains[pg1[r] + (unsigned)(fbk * FB)];
    }
    const char* src = reinterpret_cast<const char*>(A.tiles + it.tile_first + (long long)fbk * tile_elems);
    stage_t stage[L];
#pragma unroll
    for (int l = 0; l < L; ++l) stage[l] = __builtin_nontemporal_load(reinterpret_cast<const stage_t*>(src + voff[l]));

    // ---- forward, one member after the other, from the same registers
#pragma unroll
    for (int m = 0; m < NBMAX; ++m) {
      if (m < NB) {
        T2 pv[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) pv[u].x = pv[u].y = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) fma_rows(pv, stage[l], s_c[m * C::MAXK + l * NS + ks]);
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
          pv[u].x = sum_row_lanes<LPR>(pv[u].x);
          pv[u].y = sum_row_lanes<LPR>(pv[u].y);
        }
        if (lane < LPR) {
#pragma unroll
          for (int u = 0; u < VEC; ++u) s_pv[(m * kWaves + wave) * FB + f0 + u] = pv[u];
        }
      }
    }
    __syncthreads();

    // ---- per-channel stage of every (member, channel) pair
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int m = pm[r], ch = pch[r];
      if (m < NB) {
        T vr = 0, vi = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) {
          const T2 p = s_pv[(m * kWaves + wv) * FB + ch];
          vr += p.x;
          vi += p.y;
        }
        // G = g0 conj(g1)   (calibration.py:1598-1601: grgr + gigi, gigr - grgi)
        const T G_r = g0[r].x * g1[r].x + g0[r].y * g1[r].y;
        const T G_i = g0[r].y * g1[r].x - g0[r].x * g1[r].y;
        const T m_r = G_r * vr - G_i * vi;
        const T m_i = G_i * vr + G_r * vi;
        const T r_r = d_r[r] - m_r;
        const T r_i = d_i[r] - m_i;
        if (!(REG && GRAD)) loss_acc[r] += (double)(w[r] * (r_r * r_r + r_i * r_i));
        if (REG && !GRAD) {
          sr_acc[r] += (double)(w[r] * m_r);
          si_acc[r] += (double)(w[r] * m_i);
        }
        if (GRAD) {
          T e_r = (T)-2 * w[r] * r_r;
          T e_i = (T)-2 * w[r] * r_i;
          if (REG) {
            e_r += al_r[r] * w[r];
            e_i += al_i[r] * w[r];
          }
          T2 gv;  // gbar_v = conj(G) e
          gv.x = G_r * e_r + G_i * e_i;
          gv.y = G_r * e_i - G_i * e_r;
          s_gv[m * FB + ch] = gv;
          T2 q;   // gbar_G = conj(v) e
          q.x = vr * e_r + vi * e_i;
          q.y = vr * e_i - vi * e_r;
          A.q0[prow[r] + (unsigned)(fbk * FB)] = q;
        }
      }
    }
    if (GRAD) {
      __syncthreads();
      // ---- adjoint of every member: this thread's channels of its gbar_v against its rows of the tile
#pragma unroll
      for (int m = 0; m < NBMAX; ++m) {
        if (m < NB) {
          T2 gv[VEC];
#pragma unroll
          for (int u = 0; u < VEC; ++u) gv[u] = s_gv[m * FB + f0 + u];
#pragma unroll
          for (int l = 0; l < L; ++l) fma_cols(acc[m][l], stage[l], gv);
        }
      }
    } else {
      __syncthreads();  // the next tile's forward partials overwrite s_pv
    }
    // GRAD needs no barrier here: s_pv is rewritten before the next first barrier, which no wave reaches before it has left
    // this tile's per-channel stage (it sits behind the second barrier); s_gv is rewritten behind the next first barrier
  }

  // ---- epilogue: loss partial of every member (into the member's own slot: members may belong to different time slices),
  // coefficient gradients of every member.  Pair p = r * 256 + tid is (member p / FB, channel p % FB): the per-pair sums go to LDS
  // (the coefficient area is free by now) and thread m adds the FB channels of member m in order.
  __syncthreads();
  if (!(REG && GRAD)) {
    double* s_red = reinterpret_cast<double*>(smem);  // [R * kThreads] >= [NBMAX * FB]
    constexpr int NQ = REG ? 3 : 1;  // loss (, S_r, S_i), one after the other through the same area
    double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int qn = 0; qn < NQ; ++qn) {
#pragma unroll
      for (int r = 0; r < R; ++r) s_red[r * kThreads + tid] = qn == 0 ? loss_acc[r] : (qn == 1 ? sr_acc[REG && !GRAD ? r : 0] : si_acc[REG && !GRAD ? r : 0]);
      __syncthreads();
      if (tid < NB) {
        double a = 0;
        for (int ch = 0; ch < FB; ++ch) a += s_red[tid * FB + ch];
        tot[qn] = a;
      }
      __syncthreads();
    }
    if (tid < NB) {
      const size_t slot = (size_t)s_mem[tid].item * 4;
      A.part[slot + 0] = tot[0];
      A.part[slot + 1] = tot[1];
      A.part[slot + 2] = tot[2];
    }
  }
  if (GRAD) {
#pragma unroll
    for (int m = 0; m < NBMAX; ++m) {
      if (m < NB) {
        const int goff = s_mem[m].goff;
#pragma unroll
        for (int l = 0; l < L; ++l) {
#pragma unroll
          for (int sft = 1; sft < LPR; sft <<= 1) {
            acc[m][l].x += __shfl_xor(acc[m][l].x, sft, 64);
            acc[m][l].y += __shfl_xor(acc[m][l].y, sft, 64);
          }
          const int k = l * NS + ks;
          if (fq == 0 && k < nvec) {
            A.gcp0_r[goff + k] = acc[m][l].x;
            A.gcp0_i[goff + k] = acc[m][l].y;
          }
        }
      }
    }
  }
}

// ---- streaming-peak probes (cal_device_stream_peak): what the memory system delivers to the simplest possible kernel
typedef float f4_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_read_kernel(const f4_t* __restrict__ src, size_t n, float* __restrict__ sink) {
  f4_t acc = {0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * 256 * 4;
  for (size_t i = (size_t)blockIdx.x * 256 * 4 + threadIdx.x; i + 3 * 256 < n; i += stride) {
    const f4_t a = __builtin_nontemporal_load(src + i);
    const f4_t b = __builtin_nontemporal_load(src + i + 256);
    const f4_t c = __builtin_nontemporal_load(src + i + 512);
    const f4_t d = __builtin_nontemporal_load(src + i + 768);
    acc += a + b + c + d;
  }
  if (acc.x + acc.y + acc.z + acc.w == 1.2345e-30f) sink[blockIdx.x] = acc.x;  // never true for finite data: keeps the loads
}
__global__ __launch_bounds__(256) void stream_copy_kernel(const f4_t* __restrict__ src, f4_t* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void busy_clock_kernel(long long* out, int iters, float* sink) {
  const long long c0 = clock64(), w0 = wall_clock64();
  float a = threadIdx.x * 1e-3f, b = 1.0001f, c = 0.5f, d = 0.25f;
  for (int i = 0; i < iters; ++i) {
    a = __builtin_fmaf(a, b, c);
    d = __builtin_fmaf(d, b, a);
    c = __builtin_fmaf(c, b, d);
  }
  const long long c1 = clock64(), w1 = wall_clock64();
  if (a + c + d == 1.2345e-30f) sink[0] = a;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = w1 - w0;
  }
}

template <typename T> struct FbSet;
template <> struct FbSet<float> { static constexpr int fb_max = 128; static constexpr int fb_min = 8; };
template <> struct FbSet<double> { static constexpr int fb_max = 64; static constexpr int fb_min = 4; };

// ------------------------------------------------------------------------------------------------------------------
// Fitting groups of several baselines (use_redundancy / joint groups, calibration.py:173-184).
//
// Baselines of a group share one coefficient vector; those that also share the row block of the basis (a *run*: a
// redundant set) have the SAME forward product v = A c, and the adjoint is linear, A^T sum_b gbar_v_b.  So per
// (run, channel block) the tile is loaded once, the forward runs once, the per-channel stage runs for every baseline
// of the run (kThreads / FB baselines at a time, one thread per (baseline, channel)) and one adjoint takes the sum.
// With 20x fewer basis products than baselines on a redundant HERA-350 the pass is bound by the per-sample arrays.
// Work item = a range of (run, channel block) units of one group; runs are cut to at most kRunMax baselines by the host
// (64 -> 256 took 4 % off the redundant HERA-350 pass: fewer tile loads / forwards / adjoints per baseline).
constexpr int kRunMax = 256;

template <typename T, int FB, int MODE, bool REG>
__device__ __forceinline__ void process_group_item(const FusedArgs<T>& A, const Item it, unsigned char* smem, int item_idx) {
  using C = TileCfg<T, FB>;
  using T2 = vec2_t<T>;
  constexpr int VEC = C::VEC;
  constexpr int LPR = C::LPR;
  constexpr int NS = C::NS;
  constexpr int L = kMaxLoads;
  constexpr int BPT = kThreads / FB;  // baselines handled side by side in the per-channel stage
  constexpr bool FWD = (MODE != MODE_INIT);
  constexpr bool BWD = (MODE == MODE_GRAD || MODE == MODE_INIT);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fq = tid % LPR;
  const int ks = tid / LPR;
  const int f0 = fq * VEC;
  const int sub = tid / FB;
  const int ch = tid % FB;
  const int nvec = it.nvec;
  const int ntpb = A.fpad / FB;
  const int tile_elems = nvec * FB;

  T2* s_pv = reinterpret_cast<T2*>(smem);   // [2][kWaves][FB] forward partials, by unit parity
  T2* s_gv = s_pv + 2 * kWaves * FB;        // [2][FB] gbar_v summed over the run (e0 part, w part)
  T2* s_c = s_gv + 2 * FB;                  // [MAXK]
  T2* s_gvp = s_c + C::MAXK;                // [2][BPT][FB] per-sub-row sums of gbar_v
  int2* s_ant = reinterpret_cast<int2*>(s_gvp + 2 * kThreads);  // [kRunMax] antenna pairs of the current run

  typedef T stage_t __attribute__((ext_vector_type(16 / sizeof(T))));
  if (FWD) {
    for (int k = tid; k < C::MAXK; k += kThreads) {
      T2 c;
      c.x = k < nvec ? A.c_r[it.coff + k] : (T)0;
      c.y = k < nvec ? A.c_i[it.coff + k] : (T)0;
      s_c[k] = c;
    }
    __syncthreads();
  }
  unsigned voff[L];
#pragma unroll
  for (int l = 0; l < L; ++l) voff[l] = (unsigned)((min(l * NS + ks, nvec - 1) * FB + f0) * (int)sizeof(T));
  T2 acc0[L], acc1[L];
#pragma unroll
  for (int l = 0; l < L; ++l) acc0[l].x = acc0[l].y = acc1[l].x = acc1[l].y = 0;
  double loss_acc = 0.0, sr_acc = 0.0, si_acc = 0.0;

  struct Operands { T d_r, d_i, w; T2 g0, g1; };
  int cur_run = -1;
  int2 run = make_int2(0, 0);
  long long t_off = 0;
  for (int u = it.tile0; u < it.tile1; ++u) {
    const int r = u / ntpb;
    const int fbk = u - r * ntpb;
    if (r != cur_run) {
      // new run: its baseline range, its tile offset, its antenna pairs (read by the per-channel stage from LDS, so the
      // gains loads do not wait on an index load)
      cur_run = r;
      run = A.runs[it.bl0 + r];
      run.x = __builtin_amdgcn_readfirstlane(run.x);
      run.y = __builtin_amdgcn_readfirstlane(run.y);
      const long long to = A.bl_tile[run.x];
      t_off = ((long long)__builtin_amdgcn_readfirstlane((int)(to >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)to);
      if (tid < run.y - run.x) s_ant[tid] = A.bl_ant[run.x + tid];
    }
    const int nb = run.y - run.x;
    const char* src = reinterpret_cast<const char*>(A.tiles + t_off + (long long)fbk * tile_elems);
    stage_t stage[L];
#pragma unroll
    for (int l = 0; l < L; ++l) stage[l] = *reinterpret_cast<const stage_t*>(src + voff[l]);

    T2* pv_par = s_pv + (u & 1) * kWaves * FB;
    if (FWD) {
      T2 pv[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) pv[k].x = pv[k].y = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) fma_rows(pv, stage[l], s_c[l * NS + ks]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        pv[k].x = sum_row_lanes<LPR>(pv[k].x);
        pv[k].y = sum_row_lanes<LPR>(pv[k].y);
      }
      if (lane < LPR) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) pv_par[wave * FB + f0 + k] = pv[k];
      }
    }
    __syncthreads();  // forward partials and s_ant visible

    // ---- per-channel stage: thread = (baseline sub-row, channel); the forward product is the same for every baseline
    T vr = 0, vi = 0;
    if (FWD) {
#pragma unroll
      for (int wv = 0; wv < kWaves; ++wv) {
        const T2 p = pv_par[wv * FB + ch];
        vr += p.x;
        vi += p.y;
      }
    }
    auto load_operands = [&](int b) {
      Operands o;
      const int bc = min(b, nb - 1);  // sub-rows past the run re-read its last baseline and are masked below
      const long long row = (long long)(run.x + bc) * A.fpad + fbk * FB + ch;
      o.d_r = o.d_i = o.w = 0;
      o.g0.x = o.g0.y = o.g1.x = o.g1.y = 0;
      if (MODE != MODE_MODEL) {
        o.d_r = A.data_r[row];
        o.d_i = A.data_i[row];
        o.w = A.wgts[row];
      }
      if (MODE == MODE_LOSS || MODE == MODE_GRAD) {
        const int2 ant = s_ant[bc];
        o.g0 = A.gains[(long long)ant.x * A.fpad + fbk * FB + ch];
        o.g1 = A.gains[(long long)ant.y * A.fpad + fbk * FB + ch];
      }
      return o;
    };
    T2 gvsum, gwsum;
    gvsum.x = gvsum.y = gwsum.x = gwsum.y = 0;
    Operands nxt = load_operands(sub);
    for (int b0 = 0; b0 < nb; b0 += BPT) {
      const Operands o = nxt;
      if (b0 + BPT < nb) nxt = load_operands(b0 + BPT + sub);
      const int b = b0 + sub;
      const bool valid = b < nb;
      const long long row = (long long)(run.x + min(b, nb - 1)) * A.fpad + fbk * FB + ch;
      const T w = valid ? o.w : (T)0;
      if (MODE == MODE_MODEL) {
        if (valid) {
          A.model_r[row] = vr;
          A.model_i[row] = vi;
        }
      } else if (MODE == MODE_INIT) {
        const T msk = (!valid || fabs(o.w) <= (T)1e-8) ? (T)0 : (T)1;
        gvsum.x += o.d_r * msk;
        gvsum.y += o.d_i * msk;
      } else {
        const T G_r = o.g0.x * o.g1.x + o.g0.y * o.g1.y;
        const T G_i = o.g0.y * o.g1.x - o.g0.x * o.g1.y;
        const T m_r = G_r * vr - G_i * vi;
        const T m_i = G_i * vr + G_r * vi;
        const T r_r = o.d_r - m_r;
        const T r_i = o.d_i - m_i;
        loss_acc += (double)(w * (r_r * r_r + r_i * r_i));
        if (REG) {
          sr_acc += (double)(w * m_r);
          si_acc += (double)(w * m_i);
        }
        if (MODE == MODE_GRAD) {
          const T e_r = (T)-2 * w * r_r;
          const T e_i = (T)-2 * w * r_i;
          gvsum.x += G_r * e_r + G_i * e_i;
          gvsum.y += G_r * e_i - G_i * e_r;
          T2 q;
          q.x = vr * e_r + vi * e_i;
          q.y = vr * e_i - vi * e_r;
          if (valid) A.q0[row] = q;
          if (REG) {
            gwsum.x += G_r * w;
            gwsum.y += -G_i * w;
            T2 qw;
            qw.x = vr * w;
            qw.y = -vi * w;
            if (valid) A.q1[row] = qw;
          }
        }
      }
    }
    if (BWD) {
      s_gvp[sub * FB + ch] = gvsum;
      if (REG) s_gvp[kThreads + sub * FB + ch] = gwsum;
      __syncthreads();
      if (tid < FB) {
        T2 a, b2;
        a.x = a.y = b2.x = b2.y = 0;
#pragma unroll
        for (int sb = 0; sb < BPT; ++sb) {
          const T2 p = s_gvp[sb * FB + tid];
          a.x += p.x;
          a.y += p.y;
          if (REG) {
            const T2 p2 = s_gvp[kThreads + sb * FB + tid];
            b2.x += p2.x;
            b2.y += p2.y;
          }
        }
        s_gv[tid] = a;
        if (REG) s_gv[FB + tid] = b2;
      }
      __syncthreads();
      T2 gv0[VEC], gv1[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        gv0[k] = s_gv[f0 + k];
        if (REG) gv1[k] = s_gv[FB + f0 + k];
      }
#pragma unroll
      for (int l = 0; l < L; ++l) {
        fma_cols(acc0[l], stage[l], gv0);
        if (REG) fma_cols(acc1[l], stage[l], gv1);
      }
    }
    // the next unit's first barrier separates this unit's reads of s_ant / s_gv / s_gvp from their next writes, except
    // for s_ant, which a new run rewrites before that barrier:
    if (u + 1 < it.tile1 && (u + 1) / ntpb != r) __syncthreads();
  }

  // ---- item epilogue: loss partials (double), coefficient-gradient partials
  if (MODE == MODE_LOSS || MODE == MODE_GRAD) {
    __syncthreads();
    double* s_red = reinterpret_cast<double*>(s_pv);
    const double l = ldsum(loss_acc);
    const double sr = REG ? ldsum(sr_acc) : 0.0;
    const double si = REG ? ldsum(si_acc) : 0.0;
    if (lane == 0) {
      s_red[wave] = l;
      s_red[kWaves + wave] = sr;
      s_red[2 * kWaves + wave] = si;
    }
    __syncthreads();
    if (tid == 0) {
      double a = 0, b = 0, c = 0;
      for (int wv = 0; wv < kWaves; ++wv) {
        a += s_red[wv];
        b += s_red[kWaves + wv];
        c += s_red[2 * kWaves + wv];
      }
      A.part[(size_t)item_idx * 4 + 0] = a;
      A.part[(size_t)item_idx * 4 + 1] = b;
      A.part[(size_t)item_idx * 4 + 2] = c;
    }
  }
  if (BWD) {
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
      for (int sft = 1; sft < LPR; sft <<= 1) {
        acc0[l].x += __shfl_xor(acc0[l].x, sft, 64);
        acc0[l].y += __shfl_xor(acc0[l].y, sft, 64);
        if (REG) {
          acc1[l].x += __shfl_xor(acc1[l].x, sft, 64);
          acc1[l].y += __shfl_xor(acc1[l].y, sft, 64);
        }
      }
      const int k = l * NS + ks;
      if (fq == 0 && k < nvec) {
        A.gcp0_r[it.goff + k] = acc0[l].x;
        A.gcp0_i[it.goff + k] = acc0[l].y;
        if (REG) {
          A.gcp1_r[it.goff + k] = acc1[l].x;
          A.gcp1_i[it.goff + k] = acc1[l].y;
        }
      }
    }
  }
}

template <typename T, int FB>
constexpr size_t group_lds_bytes() {
  return (2 * (size_t)kWaves * FB + 2 * (size_t)FB + TileCfg<T, FB>::MAXK + 2 * (size_t)kThreads) * 2 * sizeof(T) + kRunMax * sizeof(int2) + 64;
}

#ifndef CAL_WAVES_EU
#define CAL_WAVES_EU 4
#endif
constexpr int kSmallLoads = 2;  // the narrow instance of fused_basis_kernel: blocks of at most 2 NS vectors
// FOLD: every item of the launch reads folded tiles (process_item).  (The narrow instance with the regulariser's second adjoint
// set and the mirror combinations does not fit the registers of 8 / 6 waves per SIMD without scratch: two fewer.)
template <typename T, int MODE, bool REG, int L = kMaxLoads, bool FOLD = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(L < kMaxLoads ? (sizeof(T) == 4 ? 8 : 6) - (FOLD && REG ? 2 : 0) : ((sizeof(T) == 4 && !REG) ? CAL_WAVES_EU : 1))))
void fused_basis_kernel(const FusedArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int idx = A.item_base + blockIdx.x;
  const Item it = A.items[idx];  // requested together with the stop flags: one round trip, not two
  // one time slice: its stop flags travel with the item record.  Several: the flags of the item's OWN slice, looked up inside
  // process_item beside the coefficient loads
  const DevState* st_own = nullptr;
  if (A.nslices > 1) st_own = A.state + it.slice;
  else if (A.state->done | A.state->done_after) return;
  // baselines that share tiles are processed together by fused_multi_kernel in the passes that have such a form
  if ((MODE == MODE_LOSS || MODE == MODE_GRAD) && (it.role_n & 3) != 0 && A.heads != nullptr) return;
  constexpr int FBM = FbSet<T>::fb_max;
  const int fb = 1 << it.fb_log2;
  if (fb == FBM) process_item<T, FBM, MODE, REG, L, FOLD>(A, it, smem, idx, st_own);
  else if (fb == FBM / 2) process_item<T, FBM / 2, MODE, REG, L, FOLD>(A, it, smem, idx, st_own);
  else if (fb == FBM / 4) process_item<T, FBM / 4, MODE, REG, L, FOLD>(A, it, smem, idx, st_own);
  else if (fb == FBM / 8) process_item<T, FBM / 8, MODE, REG, L, FOLD>(A, it, smem, idx, st_own);
  else process_item<T, FBM / 16, MODE, REG, L, FOLD>(A, it, smem, idx, st_own);
}

template <typename T, int MODE, bool REG>
__global__ __launch_bounds__(kThreads, 2) void fused_multi_kernel(const FusedArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int idx = A.heads[blockIdx.x];
  const Item it = A.items[idx];
  // (members of several time slices: the item runs while any of them does; a stopped member's outputs are not consumed)
  if (A.nslices == 1 && (A.state->done | A.state->done_after)) return;
  constexpr int FBM = FbSet<T>::fb_max;
  const int fb = 1 << it.fb_log2;
  if (fb == FBM) process_multi_item<T, FBM, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 2) process_multi_item<T, FBM / 2, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 4) process_multi_item<T, FBM / 4, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 8) process_multi_item<T, FBM / 8, MODE, REG>(A, it, smem, idx);
  else process_multi_item<T, FBM / 16, MODE, REG>(A, it, smem, idx);
}

template <typename T, int MODE, bool REG>
__global__ __launch_bounds__(kThreads) void fused_group_kernel(const FusedArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int idx = A.item_base + blockIdx.x;
  const Item it = A.items[idx];
  const DevState* st = A.state;
  if (A.nslices > 1) st += it.slice;
  if (st->done | st->done_after) return;
  constexpr int FBM = FbSet<T>::fb_max;
  const int fb = 1 << it.fb_log2;
  if (fb == FBM) process_group_item<T, FBM, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 2) process_group_item<T, FBM / 2, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 4) process_group_item<T, FBM / 4, MODE, REG>(A, it, smem, idx);
  else if (fb == FBM / 8) process_group_item<T, FBM / 8, MODE, REG>(A, it, smem, idx);
  else process_group_item<T, FBM / 16, MODE, REG>(A, it, smem, idx);
}

// ---- sum the partial coefficient gradients of multi-item groups: gc[n] = sum_q gcp[goff_q + k]
template <typename T>
__global__ void coeff_partial_reduce_kernel(const T* __restrict__ gcp_r, const T* __restrict__ gcp_i, T* __restrict__ gc_r,
                                            T* __restrict__ gc_i, const int* __restrict__ coef_grp,
                                            const int* __restrict__ grp_coff, const int* __restrict__ grp_item_ptr,
                                            const int* __restrict__ item_goff, int ncoef, const DevState* st, const SliceMap M) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= ncoef) return;
  if (M.nslices > 1) st += slice_of_coef(M, n);
  if (st->done | st->done_after) return;
  const int g = coef_grp[n];
  const int k = n - grp_coff[g];
  T a = 0, b = 0;
  for (int q = grp_item_ptr[g]; q < grp_item_ptr[g + 1]; ++q) {
    a += gcp_r[item_goff[q] + k];
    b += gcp_i[item_goff[q] + k];
  }
  gc_r[n] = a;
  gc_i[n] = b;
}

// Sum of the loss partials (chi^2, S_r, S_i) of ONE time slice by one 256-thread block, in a fixed order: thread t takes entries
// t, t + 256, ... of the slice's list; a butterfly over the 64 lanes of each wave; the four waves in order.  Shared by
// gain_grad_kernel's last blocks and by every block of step_tail_kernel (the launch forms of a step must agree bit for bit).
// Entry i of the list is part[idx ? idx[p0 + i] : p0 + i] (idx: SliceMap::part_idx, nullptr with one slice), n entries.
// x: the caller's loads of entry threadIdx.x (issued early so that they travel together with its other loads), valid when
// threadIdx.x < n.  Result in out[0..2] on every thread; sh: 12 doubles of LDS.
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, const int* __restrict__ idx, int p0, int n, const double x[3],
                                             double* sh, double out[3]) {
  const int tid = threadIdx.x;
  double a = 0, b = 0, c = 0;
  if (tid < n) {
    a = x[0];
    b = x[1];
    c = x[2];
  }
  for (int i = tid + 256; i < n; i += 256) {
    const size_t e = idx ? (size_t)idx[p0 + i] : (size_t)(p0 + i);
    a += part[e * 4 + 0];
    b += part[e * 4 + 1];
    c += part[e * 4 + 2];
  }
  a = ldsum(a);
  b = ldsum(b);
  c = ldsum(c);
  if ((tid & 63) == 0) {
    sh[(tid >> 6) * 3 + 0] = a;
    sh[(tid >> 6) * 3 + 1] = b;
    sh[(tid >> 6) * 3 + 2] = c;
  }
  __syncthreads();
  out[0] = ((sh[0] + sh[3]) + sh[6]) + sh[9];
  out[1] = ((sh[1] + sh[4]) + sh[7]) + sh[10];
  out[2] = ((sh[2] + sh[5]) + sh[8]) + sh[11];
}
// the entries of slice t: first entry, count (one slice: all nparts), and this thread's early load of entry threadIdx.x
__device__ __forceinline__ void slice_partials(const SliceMap& M, int t, int nparts, const double* __restrict__ part, int& p0, int& n, double x[3]) {
  p0 = 0;
  n = nparts;
  if (M.nslices > 1) {
    p0 = M.part_ptr[t];
    n = M.part_ptr[t + 1] - p0;
  }
  x[0] = x[1] = x[2] = 0;
  if ((int)threadIdx.x < n) {
    const size_t e = M.part_idx ? (size_t)M.part_idx[p0 + threadIdx.x] : (size_t)(p0 + threadIdx.x);
    x[0] = part[e * 4 + 0];
    x[1] = part[e * 4 + 1];
    x[2] = part[e * 4 + 2];
  }
}

// The per-antenna reduction shared by gain_grad_kernel and step_tail_kernel (ONE body: the two launch forms of a step must
// agree bit for bit).  The calling block is 256 threads = 4 segments of the antenna's sorted baseline list; lane = CPL adjacent
// channels starting at f.  Returns true on the lanes of segment 0 that own channels (f < fpad): they hold the sums
// s0 (and s1, s2 with the regulariser), combined over the four segments in fixed order through s_part.
template <typename T, bool REG>
__device__ __forceinline__ bool antenna_sums(const vec2_t<T>* __restrict__ q0, const vec2_t<T>* __restrict__ q1, const vec2_t<T>* __restrict__ gains,
                                             const int* __restrict__ ant_ptr, const int2* __restrict__ ant_ent, int a, int f, int fpad,
                                             T (*s_part)[3][64][2 * (16 / (int)sizeof(vec2_t<T>) > 0 ? 16 / (int)sizeof(vec2_t<T>) : 1)],
                                             T* s0, T* s1, T* s2) {
  constexpr int CPL = 16 / (int)sizeof(vec2_t<T>) > 0 ? 16 / (int)sizeof(vec2_t<T>) : 1;
  typedef T vec_t __attribute__((ext_vector_type(2 * CPL)));
  const int lane = threadIdx.x & 63;
  const int seg = threadIdx.x >> 6;
  const bool ok = f < fpad;  // fpad is a multiple of CPL
#pragma unroll
  for (int c = 0; c < 2 * CPL; ++c) s0[c] = s1[c] = s2[c] = 0;
  const int e0 = ant_ptr[a], e1 = ant_ptr[a + 1];
  const int per = (e1 - e0 + 3) >> 2;
  const int eb = e0 + seg * per, ee = min(e1, eb + per);
  if (ok) {
#pragma unroll 8  // eight rows' loads in flight per wave (4: 25 us slower behind the streaming kernel at HERA-350; one channel per lane: 50 us slower)
    for (int e = eb; e < ee; ++e) {
      const int2 ent = ant_ent[e];  // (bl * 2 + role, other antenna): wave-uniform
      const int bl = ent.x >> 1;
      const int role = ent.x & 1;
      const vec_t q = *reinterpret_cast<const vec_t*>(q0 + (long long)bl * fpad + f);
      const vec_t go = *reinterpret_cast<const vec_t*>(gains + (long long)ent.y * fpad + f);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const T qr = q[2 * c], qi = role ? -q[2 * c + 1] : q[2 * c + 1];
        s0[2 * c] = fma_(-qi, go[2 * c + 1], fma_(qr, go[2 * c], s0[2 * c]));
        s0[2 * c + 1] = fma_(qi, go[2 * c], fma_(qr, go[2 * c + 1], s0[2 * c + 1]));
      }
      if (REG) {
        const vec_t p = *reinterpret_cast<const vec_t*>(q1 + (long long)bl * fpad + f);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const T pr = p[2 * c], pi = p[2 * c + 1];
          if (role == 0) {
            s1[2 * c] = fma_(-pi, go[2 * c + 1], fma_(pr, go[2 * c], s1[2 * c]));
            s1[2 * c + 1] = fma_(pi, go[2 * c], fma_(pr, go[2 * c + 1], s1[2 * c + 1]));
          } else {
            s2[2 * c] = fma_(pi, go[2 * c + 1], fma_(pr, go[2 * c], s2[2 * c]));
            s2[2 * c + 1] = fma_(-pi, go[2 * c], fma_(pr, go[2 * c + 1], s2[2 * c + 1]));
          }
        }
      }
    }
  }
  if (seg > 0) {
#pragma unroll
    for (int c = 0; c < 2 * CPL; ++c) {
      s_part[seg - 1][0][lane][c] = s0[c];
      if (REG) {
        s_part[seg - 1][1][lane][c] = s1[c];
        s_part[seg - 1][2][lane][c] = s2[c];
      }
    }
  }
  __syncthreads();
  if (seg == 0 && ok) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
      for (int c = 0; c < 2 * CPL; ++c) {
        s0[c] += s_part[g][0][lane][c];
        if (REG) {
          s1[c] += s_part[g][1][lane][c];
          s2[c] += s_part[g][2][lane][c];
        }
      }
    }
    return true;
  }
  return false;
}

// ---- per-antenna segmented reduction of gbar_G (gradient of the gain gathers) + loss partial sums.
// block = (antenna a, 64 * CPL channels); the antenna's baselines are a sorted CSR list (entry = bl * 2 + role, other
// antenna) split into 4 segments, one per wave; lane = CPL adjacent channels (16-byte loads of gbar_G and of the other
// antenna's gains); the 4 partial sums are combined through LDS in fixed order (bitwise reproducible, no float atomics).
// grad g_a[f] = sum_{role 0} Q[bl][f] g_other[f] + sum_{role 1} conj(Q[bl][f]) g_other[f]
template <typename T, bool REG>
__global__ __launch_bounds__(256) void gain_grad_kernel(const vec2_t<T>* __restrict__ q0, const vec2_t<T>* __restrict__ q1,
                                                         const vec2_t<T>* __restrict__ gains, const int* __restrict__ ant_ptr,
                                                         const int2* __restrict__ ant_ent, vec2_t<T>* __restrict__ r0,
                                                         vec2_t<T>* __restrict__ r1, vec2_t<T>* __restrict__ r2, int nants,
                                                         int fpad, const double* __restrict__ part, int nitems,
                                                         double* __restrict__ scal, const DevState* st, const SliceMap M) {
  using T2 = vec2_t<T>;
  constexpr int CPL = 16 / (int)sizeof(T2) > 0 ? 16 / (int)sizeof(T2) : 1;  // channels per lane: 2 (fp32), 1 (fp64)
  typedef T vec_t __attribute__((ext_vector_type(2 * CPL)));
  const int cblocks = (fpad + 64 * CPL - 1) / (64 * CPL);
  const int nb_main = nants * cblocks;
  if ((int)blockIdx.x >= nb_main) {
    // the last nslices blocks: deterministic sum of the loss partials of one time slice each -> scal[4 t + 0..2]
    const int t = (int)blockIdx.x - nb_main;
    if (st[t].done | st[t].done_after) return;
    __shared__ double sh[12];
    double x[3], tot[3];
    int p0, n;
    slice_partials(M, t, nitems, part, p0, n, x);
    sum_partials(part, M.part_idx, p0, n, x, sh, tot);
    if (threadIdx.x == 0) {
      scal[4 * t + 0] = tot[0];
      scal[4 * t + 1] = tot[1];
      scal[4 * t + 2] = tot[2];
    }
    return;
  }
  __shared__ T s_part[3][3][64][2 * CPL];  // [segment 1..3][sum 0..2][lane][components]
  // channel-block-major grid: the two antennas of a baseline read the same piece of its gbar_G row, and with all the
  // antennas of one channel block next to each other in dispatch order the second read finds it in the Infinity Cache
  // (antenna-major, the two reads of a row are up to the whole array apart: they both came from HBM, 0.30 -> 0.2 ms
  // behind the streaming kernel at HERA-350)
  const int cb = blockIdx.x / nants;
  const int a = blockIdx.x - cb * nants;
  const int lane = threadIdx.x & 63;
  const int f = (cb * 64 + lane) * CPL;
  if (M.nslices > 1) st += a / M.na_slice;
  if (st->done | st->done_after) {
    // a stopped slice of several: its gradient rows are still part of the exchange payload -- keep them zero rather than stale
    // (an all-reduce in place would multiply what is left there by the number of ranks, step after step)
    if (M.nslices > 1 && threadIdx.x < 64 && f < fpad) {
      vec_t z;
#pragma unroll
      for (int c = 0; c < 2 * CPL; ++c) z[c] = 0;
      const long long idx = (long long)a * fpad + f;
      *reinterpret_cast<vec_t*>(r0 + idx) = z;
      if (REG) {
        *reinterpret_cast<vec_t*>(r1 + idx) = z;
        *reinterpret_cast<vec_t*>(r2 + idx) = z;
      }
    }
    return;
  }
  T s0[2 * CPL], s1[2 * CPL], s2[2 * CPL];
  const bool mine = antenna_sums<T, REG>(q0, q1, gains, ant_ptr, ant_ent, a, f, fpad, s_part, s0, s1, s2);
  if (mine) {
    vec_t o0, o1, o2;
#pragma unroll
    for (int c = 0; c < 2 * CPL; ++c) {
      o0[c] = s0[c];
      o1[c] = s1[c];
      o2[c] = s2[c];
    }
    const long long idx = (long long)a * fpad + f;
    *reinterpret_cast<vec_t*>(r0 + idx) = o0;
    if (REG) {
      *reinterpret_cast<vec_t*>(r1 + idx) = o1;
      *reinterpret_cast<vec_t*>(r2 + idx) = o2;
    }
  }
}

// ---- loop bookkeeping of calibration.py:699-717 on the device: one function for the three kernels that run it
// (finalize_kernel: large problems, one thread; step_update_kernel / step_tail_kernel: thread 0 of every block).
// s: the state BEFORE this step, advanced in place; l0, l1, l2: the reduced loss sums (chi^2, S_r, S_i).  Returns whether the
// step updates the parameters.  `writer` records the loss (one block does).
__device__ inline bool advance_state(DevState& s, double l0, double l1, double l2, bool writer, double* __restrict__ losses, int losses_cap,
                                     bool apply_update) {
  if (s.done) return false;
  if (s.done_after) {
    s.done = 1;
    return false;
  }
  double loss = l0;
  if (s.reg) {
    s.s_r = l1;
    s.s_i = l2;
    const double dr = l1 - s.prior_r, di = l2 - s.prior_i;
    loss += dr * dr + di * di;
    s.alpha_r = 2.0 * dr;
    s.alpha_i = 2.0 * di;
  }
  s.loss = loss;
  s.improved = 0;
  if (!apply_update) return false;
  if (!(loss == loss) || loss > 1.7e308 || loss < -1.7e308) {
    // non-finite loss: never silently continued: stop before this step's update
    s.nonfinite = 1;
    s.done = 1;
    return false;
  }
  s.t += 1;
  s.nupdates += 1;
  s.b1t *= s.beta1;
  s.b2t *= s.beta2;
  s.bc1 = 1.0 - s.b1t;
  s.lr_t = s.lr * sqrt(1.0 - s.b2t) / s.bc1;
  s.lr_u = s.lr / s.bc1;
  // the step's update coefficients (Keras OptimizerV2 semantics; optimizer_step reads them)
  s.k[0] = s.lr;
  switch (s.opt) {
    case OPT_ADAM: s.k[0] = s.lr_t; break;
    case OPT_ADAMAX: s.k[0] = s.lr_u; break;
    case OPT_SGD: s.k[1] = s.momentum; s.k[2] = s.nesterov ? 1.0 : 0.0; break;
    case OPT_RMSPROP: s.k[1] = s.rho; s.k[2] = s.momentum; break;
    case OPT_ADADELTA: s.k[1] = s.rho; break;
    case OPT_FTRL: s.k[1] = s.ftrl[0]; s.k[2] = s.ftrl[1]; s.k[3] = s.ftrl[2]; s.k[4] = s.ftrl[3]; break;
    case OPT_LAMB: s.k[1] = 1.0 - s.b1t; s.k[2] = 1.0 - s.b2t; s.k[3] = s.ftrl[0]; break;  // bias corrections, weight decay rate
    case OPT_NADAM: {
      const double mu_t = s.beta1 * (1.0 - 0.5 * pow(0.96, 0.004 * (double)s.t));
      const double mu_t1 = s.beta1 * (1.0 - 0.5 * pow(0.96, 0.004 * (double)(s.t + 1)));
      const double sched_new = s.nadam_sched * mu_t, sched_next = sched_new * mu_t1;
      s.nadam_sched = sched_new;
      s.k[1] = 1.0 - sched_new;
      s.k[2] = 1.0 - sched_next;
      s.k[3] = 1.0 - s.b2t;
      s.k[4] = 1.0 - mu_t;
      s.k[5] = mu_t1;
      break;
    }
    default: break;
  }
  if (s.record) {
    if (writer && s.n_recorded < losses_cap) losses[s.n_recorded] = loss;
    s.n_recorded += 1;
    // The reference compares the values loss.numpy() returns (:702, :712): float32 numbers in a float32 fit, so such a
    // fit stops once its loss stagnates in float32 (difference exactly 0 < tol).  The loss itself is accumulated and
    // recorded in double here; only the two comparisons see it rounded.
    const double lc = s.f32 ? (double)(float)loss : loss;
    if (s.use_min && lc < s.min_loss) {
      s.min_loss = lc;
      s.improved = 1;
    }
    if (s.n_recorded_total >= 1 && fabs(lc - s.prev_loss) < s.tol) s.done_after = 1;
    s.prev_loss = lc;
    s.n_recorded_total += 1;
  }
  return true;
}

// ---- one parameter's update: tf.keras.optimizers.* as of OptimizerV2 (TensorFlow 2.4 - 2.10, the versions the reference
// was written against; calibration.py:17-27, :571, :667), applied to the re and im variables independently (:596-603).
// pi: parameter, gi: gradient, m / v: the optimizer's two slots (zero at the start unless noted), k: DevState::k of the step.
//   Adam     m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g^2; p -= k0 m / (sqrt(v) + eps), k0 = lr sqrt(1 - b2^t) / (1 - b1^t)
//   Adamax   m likewise; v <- max(b2 v, |g|); p -= k0 m / (v + eps), k0 = lr / (1 - b1^t)       (epsilon outside the bias correction)
//   SGD      k1 = momentum: 0 -> p -= lr g; else m <- k1 m - lr g, p += m (nesterov: p += k1 m - lr g)
//   RMSprop  v <- rho v + (1 - rho) g^2; momentum 0 -> p -= lr g / (sqrt(v) + eps); else m <- mom m + lr g / sqrt(v + eps), p -= m
//   Adagrad  v <- v + g^2 (v starts at initial_accumulator_value); p -= lr g / (sqrt(v) + eps)
//   Adadelta v <- rho v + (1 - rho) g^2; u = sqrt(m + eps) / sqrt(v + eps) g; p -= lr u; m <- rho m + (1 - rho) u^2
//   Ftrl     (ResourceApplyFtrl[V2]; m = linear, v = accumulator from initial_accumulator_value; k1 = lr_power, k2 = l1, k3 = l2 + beta / (2 lr),
//            k4 = l2_shrinkage)  v' = v + g^2; sigma = (v'^-k1 - v^-k1) / lr; m += g + 2 k4 p - sigma p; p = |m| > k2 ? (sign(m) k2 - m) / (v'^-k1 / lr + 2 k3) : 0
//   Nadam    g' = g / k1; m <- b1 m + (1 - b1) g; m' = m / k2; v <- b2 v + (1 - b2) g^2; v' = v / k3; p -= lr (k4 g' + k5 m') / (sqrt(v') + eps)
template <typename T>
struct StepCoef { T b1, b2, eps, k[6]; int opt; };
template <typename T> __device__ __forceinline__ StepCoef<T> step_coef(const DevState& s) {
  StepCoef<T> c;
  c.b1 = (T)s.beta1; c.b2 = (T)s.beta2; c.eps = (T)s.eps; c.opt = s.opt;
#pragma unroll
  for (int i = 0; i < 6; ++i) c.k[i] = (T)s.k[i];
  return c;
}
template <typename T> __device__ __forceinline__ T optimizer_step(T pi, T gi, T& mi_io, T& vi_io, const StepCoef<T>& c) {
#pragma clang fp contract(off)
  switch (c.opt) {
    case OPT_ADAM: {
      const T mi = c.b1 * mi_io + ((T)1 - c.b1) * gi;
      const T vi = c.b2 * vi_io + ((T)1 - c.b2) * gi * gi;
      vi_io = vi;
      mi_io = mi;
      return pi - c.k[0] * mi / (sqrt(vi) + c.eps);
    }
    case OPT_ADAMAX: {
      const T mi = c.b1 * mi_io + ((T)1 - c.b1) * gi;
      const T ui = fmax(c.b2 * vi_io, fabs(gi));
      vi_io = ui;
      mi_io = mi;
      return pi - c.k[0] * mi / (ui + c.eps);
    }
    case OPT_SGD: {
      if (c.k[1] == (T)0) return pi - c.k[0] * gi;
      const T acc = c.k[1] * mi_io - c.k[0] * gi;
      mi_io = acc;
      return c.k[2] != (T)0 ? pi + (c.k[1] * acc - c.k[0] * gi) : pi + acc;
    }
    case OPT_RMSPROP: {
      const T rms = c.k[1] * vi_io + ((T)1 - c.k[1]) * gi * gi;
      vi_io = rms;
      if (c.k[2] == (T)0) return pi - c.k[0] * gi / (sqrt(rms) + c.eps);
      const T mom = c.k[2] * mi_io + c.k[0] * gi / sqrt(rms + c.eps);
      mi_io = mom;
      return pi - mom;
    }
    case OPT_ADAGRAD: {
      const T acc = vi_io + gi * gi;
      vi_io = acc;
      return pi - c.k[0] * gi / (sqrt(acc) + c.eps);
    }
    case OPT_ADADELTA: {
      const T acc = c.k[1] * vi_io + ((T)1 - c.k[1]) * gi * gi;
      vi_io = acc;
      const T upd = sqrt(mi_io + c.eps) / sqrt(acc + c.eps) * gi;
      mi_io = c.k[1] * mi_io + ((T)1 - c.k[1]) * upd * upd;
      return pi - c.k[0] * upd;
    }
    case OPT_FTRL: {
      const T acc = vi_io, acc_new = acc + gi * gi;
      const bool half = c.k[1] == (T)-0.5;  // the special case of the TensorFlow kernel: square roots instead of pow
      const T pn = half ? sqrt(acc_new) : pow(acc_new, -c.k[1]);
      const T po = half ? sqrt(acc) : pow(acc, -c.k[1]);
      const T g_shr = gi + (T)2 * c.k[4] * pi;  // l2 shrinkage enters the linear term only
      const T lin = mi_io + g_shr - (pn - po) / c.k[0] * pi;
      mi_io = lin;
      vi_io = acc_new;
      const T quad = pn / c.k[0] + (T)2 * c.k[3];
      const T sgn = lin > (T)0 ? (T)1 : (lin < (T)0 ? (T)-1 : (T)0);
      return fabs(lin) > c.k[2] ? (sgn * c.k[2] - lin) / quad : (T)0;
    }
    default: {  // OPT_NADAM
      const T g_prime = gi / c.k[1];
      const T mi = c.b1 * mi_io + ((T)1 - c.b1) * gi;
      const T m_prime = mi / c.k[2];
      const T vi = c.b2 * vi_io + ((T)1 - c.b2) * gi * gi;
      const T v_prime = vi / c.k[3];
      mi_io = mi;
      vi_io = vi;
      return pi - c.k[0] * (c.k[4] * g_prime + c.k[5] * m_prime) / (sqrt(v_prime) + c.eps);
    }
  }
}

__global__ void finalize_kernel(DevState* st, const double* __restrict__ scal, double* __restrict__ losses, int losses_cap,
                                int apply_update, int nslices) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per time slice
  if (t >= nslices) return;
  DevState s = st[t];
  advance_state(s, scal[4 * t + 0], scal[4 * t + 1], scal[4 * t + 2], true, losses + (size_t)t * losses_cap, losses_cap, apply_update != 0);
  st[t] = s;
}

// Nadam's momentum schedule after t updates, as advance_state builds it (cal_solver_set_moments: resume)
__global__ void nadam_sched_kernel(double beta1, long long t, double* __restrict__ out) {
  double sched = 1.0;
  for (long long k = 1; k <= t; ++k) sched *= beta1 * (1.0 - 0.5 * pow(0.96, 0.004 * (double)k));
  *out = sched;
}

// ---- "sum" regulariser, two-pass form (dense path): alpha = 2 (S - P) from the reduced sums of a loss-only pass
__global__ void alpha_kernel(DevState* st, const double* __restrict__ scal, int nslices) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nslices) return;
  if (st[t].done | st[t].done_after) return;
  st[t].alpha_r = 2.0 * (scal[4 * t + 1] - st[t].prior_r);
  st[t].alpha_i = 2.0 * (scal[4 * t + 2] - st[t].prior_i);
}

// ---- "sum" regulariser: fold the alpha-weighted parts into the gradients once alpha is known.  The two folds are functions
// of their own because two kernels apply them (combine_* here, step_tail_kernel) and must round identically.
template <typename T> __device__ __forceinline__ void fold_gain(T& ax, T& ay, T bx, T by, T cx, T cy, T ar, T ai) {
#pragma clang fp contract(off)
  // + alpha * r1 + conj(alpha) * r2
  ax += ar * bx - ai * by + ar * cx + ai * cy;
  ay += ar * by + ai * bx + ar * cy - ai * cx;
}
// one real component of g0 + alpha g1 (complex): `same` is g1's component of the same plane, `other` that of the other plane
template <typename T> __device__ __forceinline__ T fold_coeff(T g0, T same, T other, T ar, T ai, bool imag) {
#pragma clang fp contract(off)
  return imag ? g0 + (ar * same + ai * other) : g0 + (ar * same - ai * other);
}
template <typename T>
__global__ void combine_gain_kernel(vec2_t<T>* __restrict__ r0, const vec2_t<T>* __restrict__ r1,
                                    const vec2_t<T>* __restrict__ r2, int n, const DevState* st, const SliceMap M, int fpad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (M.nslices > 1) st += (i / fpad) / M.na_slice;
  if (st->done) return;
  const T ar = (T)st->alpha_r, ai = (T)st->alpha_i;
  vec2_t<T> a = r0[i];
  const vec2_t<T> b = r1[i], c = r2[i];
  fold_gain(a.x, a.y, b.x, b.y, c.x, c.y, ar, ai);
  r0[i] = a;
}

template <typename T>
__global__ void combine_coeff_kernel(T* __restrict__ g0_r, T* __restrict__ g0_i, const T* __restrict__ g1_r,
                                     const T* __restrict__ g1_i, int n, const DevState* st, const SliceMap M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (M.nslices > 1) st += slice_of_coef(M, i);
  if (st->done) return;
  const T ar = (T)st->alpha_r, ai = (T)st->alpha_i;
  g0_r[i] = fold_coeff(g0_r[i], g1_r[i], g1_i[i], ar, ai, false);
  g0_i[i] = fold_coeff(g0_i[i], g1_i[i], g1_r[i], ar, ai, true);
}

// ---- the optimizer update on flat real arrays (optimizer_step), both parameter sets in one launch (one launch less per
// step matters for problems whose whole step is ~20 us): blocks [0, nblk_a) update set a (the gains), the rest set b (the
// coefficients).
template <typename T>
struct AdamSet { T* p; const T* g; T* m; T* v; T* snap; long long n; };
// slice of element i of the flat gain array [nants][fpad][2] / of the flat coefficient planes [2][ncoef]
__device__ __forceinline__ int slice_of_gain_real(const SliceMap& M, long long i, int fpad) { return (int)(i / (2LL * fpad)) / M.na_slice; }
__device__ __forceinline__ int slice_of_coef_real(const SliceMap& M, long long i, int ncoef) { return slice_of_coef(M, (int)(i >= ncoef ? i - ncoef : i)); }

// A thread takes kAdamVec<T> = 16 bytes of consecutive elements of every array (four 16-byte loads, three or four 16-byte stores per
// thread; one element per thread ran the same update at 4.3 TB/s of the 8).  The arithmetic is per element and unchanged; a thread
// whose elements straddle two time slices, the end of the set, or arrays that are not 16-byte aligned takes them one by one.
template <typename T> constexpr int kAdamVec = 16 / (int)sizeof(T);
template <typename T>
__global__ __launch_bounds__(256) void adam2_kernel(const AdamSet<T> a, const AdamSet<T> b, int nblk_a, const DevState* st, const SliceMap M,
                                                    int fpad, int ncoef) {
  constexpr int V = kAdamVec<T>;
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const bool first = (int)blockIdx.x < nblk_a;
  const AdamSet<T>& S = first ? a : b;
  const long long i0 = ((long long)(first ? blockIdx.x : blockIdx.x - nblk_a) * blockDim.x + threadIdx.x) * V;
  if (i0 >= S.n) return;
  const int t0 = M.nslices > 1 ? (first ? slice_of_gain_real(M, i0, fpad) : slice_of_coef_real(M, i0, ncoef)) : 0;
  bool together = i0 + V <= S.n;
  if (together && M.nslices > 1) together = t0 == (first ? slice_of_gain_real(M, i0 + V - 1, fpad) : slice_of_coef_real(M, i0 + V - 1, ncoef));
  const unsigned long long align = (unsigned long long)S.p | (unsigned long long)S.g | (unsigned long long)S.m | (unsigned long long)S.v | (unsigned long long)S.snap;
  if (together && (align & 15) == 0) {
    const DevState* s = st + t0;
    if (s->done) return;
    const StepCoef<T> c = step_coef<T>(*s);
    vec_t p = *reinterpret_cast<const vec_t*>(S.p + i0);
    const vec_t g = *reinterpret_cast<const vec_t*>(S.g + i0);
    vec_t m = *reinterpret_cast<const vec_t*>(S.m + i0), v = *reinterpret_cast<const vec_t*>(S.v + i0);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      T mi = m[e], vi = v[e];
      p[e] = optimizer_step<T>(p[e], g[e], mi, vi, c);
      m[e] = mi;
      v[e] = vi;
    }
    *reinterpret_cast<vec_t*>(S.m + i0) = m;
    *reinterpret_cast<vec_t*>(S.v + i0) = v;
    *reinterpret_cast<vec_t*>(S.p + i0) = p;
    if (s->improved) *reinterpret_cast<vec_t*>(S.snap + i0) = p;
    return;
  }
  for (long long i = i0; i < i0 + V && i < S.n; ++i) {
    const DevState* s = st;
    if (M.nslices > 1) s += first ? slice_of_gain_real(M, i, fpad) : slice_of_coef_real(M, i, ncoef);
    if (s->done) continue;
    const StepCoef<T> c = step_coef<T>(*s);
    T mi = S.m[i], vi = S.v[i];
    const T pi = optimizer_step<T>(S.p[i], S.g[i], mi, vi, c);
    S.m[i] = mi;
    S.v[i] = vi;
    S.p[i] = pi;
    if (s->improved) S.snap[i] = pi;
  }
}

// ---- LAMB (tensorflow_addons.optimizers.LAMB, calibration.py:26): Adam moments, then a trust ratio PER VARIABLE -- the reference's
// variables are g_r, g_i and one fg_r[chunk], fg_i[chunk] per chunk (calibration.py:596-603) --
//   m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g^2; u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd p;
//   ratio = |p| > 0 and |u| > 0 ? |p| / |u| : 1 (2-norms over the variable);  p <- p - lr ratio u.
// Four launches: moments + u (u overwrites the gradient), per-variable partial norms (LAMB_NSEG segments per variable, fixed
// order), the ratios, the update.  A variable is a strided run of one of the two parameter arrays.
struct LambVar { long long off; long long n; int stride; int set; };  // set 0: gains [nants][fpad][2], 1: coefficient planes
constexpr int kLambSeg = 64;
template <typename T>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const AdamSet<T> a, const AdamSet<T> b, int nblk_a, const DevState* st, const SliceMap M,
                                                           int fpad, int ncoef, T* __restrict__ ua, T* __restrict__ ub) {
#pragma clang fp contract(off)
  const bool first = (int)blockIdx.x < nblk_a;
  const AdamSet<T>& S = first ? a : b;
  T* u_out = first ? ua : ub;
  const long long i = (long long)(first ? blockIdx.x : blockIdx.x - nblk_a) * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  if (M.nslices > 1) st += first ? slice_of_gain_real(M, i, fpad) : slice_of_coef_real(M, i, ncoef);
  if (st->done) return;
  const StepCoef<T> c = step_coef<T>(*st);
  const T g = S.g[i];
  const T mi = c.b1 * S.m[i] + ((T)1 - c.b1) * g;
  const T vi = c.b2 * S.v[i] + ((T)1 - c.b2) * g * g;
  S.m[i] = mi;
  S.v[i] = vi;
  u_out[i] = (mi / c.k[1]) / (sqrt(vi / c.k[2]) + c.eps) + c.k[3] * S.p[i];
}
template <typename T>
__global__ __launch_bounds__(256) void lamb_norm_kernel(const LambVar* __restrict__ vars, const T* __restrict__ pa, const T* __restrict__ ua,
                                                        const T* __restrict__ pb, const T* __restrict__ ub, double* __restrict__ partial) {
  const int v = blockIdx.x / kLambSeg, seg = blockIdx.x - v * kLambSeg;
  const LambVar V = vars[v];
  const T* p = V.set ? pb : pa;
  const T* u = V.set ? ub : ua;
  const long long per = (V.n + kLambSeg - 1) / kLambSeg;
  const long long e0 = seg * per, e1 = e0 + per < V.n ? e0 + per : V.n;
  double sw = 0, su = 0;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const long long idx = V.off + e * V.stride;
    const double x = (double)p[idx], y = (double)u[idx];
    sw += x * x;
    su += y * y;
  }
  __shared__ double sh[8];
  sw = ldsum(sw);
  su = ldsum(su);
  if ((threadIdx.x & 63) == 0) {
    sh[(threadIdx.x >> 6) * 2 + 0] = sw;
    sh[(threadIdx.x >> 6) * 2 + 1] = su;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[(size_t)blockIdx.x * 2 + 0] = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    partial[(size_t)blockIdx.x * 2 + 1] = ((sh[1] + sh[3]) + sh[5]) + sh[7];
  }
}
// (several ranks: the coefficient variables' sums go through `glob`, all-reduced between lamb_fold_kernel and lamb_ratio_kernel: local
// variable k of plane p -> glob[p * nslot + slot[k]]; the gain variables [0, ngvar) are replicated and keep their local sums)
__global__ void lamb_fold_kernel(const double* __restrict__ partial, double* __restrict__ glob, const int* __restrict__ slot, int ngvar, int ncvar,
                                 int nslot) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;  // (plane, local coefficient variable)
  if (c >= 2 * ncvar) return;
  const int plane = c / ncvar, k = c - plane * ncvar;
  const size_t v = (size_t)ngvar + c;
  double sw = 0, su = 0;
  for (int s = 0; s < kLambSeg; ++s) {
    sw += partial[(v * kLambSeg + s) * 2 + 0];
    su += partial[(v * kLambSeg + s) * 2 + 1];
  }
  glob[((size_t)plane * nslot + slot[k]) * 2 + 0] = sw;
  glob[((size_t)plane * nslot + slot[k]) * 2 + 1] = su;
}
__global__ void lamb_ratio_kernel(const double* __restrict__ partial, double* __restrict__ ratio, int nvar, const double* __restrict__ glob,
                                  const int* __restrict__ slot, int ngvar, int ncvar, int nslot) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nvar) return;
  double sw = 0, su = 0;
  if (glob && v >= ngvar) {
    const int plane = (v - ngvar) / ncvar, k = (v - ngvar) - plane * ncvar;
    sw = glob[((size_t)plane * nslot + slot[k]) * 2 + 0];
    su = glob[((size_t)plane * nslot + slot[k]) * 2 + 1];
  } else {
    for (int s = 0; s < kLambSeg; ++s) {
      sw += partial[((size_t)v * kLambSeg + s) * 2 + 0];
      su += partial[((size_t)v * kLambSeg + s) * 2 + 1];
    }
  }
  const double wn = sqrt(sw), un = sqrt(su);
  ratio[v] = wn > 0.0 ? (un > 0.0 ? wn / un : 1.0) : 1.0;
}
template <typename T>
__global__ __launch_bounds__(256) void lamb_apply_kernel(const AdamSet<T> a, const AdamSet<T> b, int nblk_a, const DevState* st, const SliceMap M,
                                                         int fpad, int ncoef, const T* __restrict__ ua, const T* __restrict__ ub,
                                                         const double* __restrict__ ratio, const int* __restrict__ cvar_ptr, int ncvar) {
#pragma clang fp contract(off)
  const bool first = (int)blockIdx.x < nblk_a;
  const AdamSet<T>& S = first ? a : b;
  const long long i = (long long)(first ? blockIdx.x : blockIdx.x - nblk_a) * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  int var;
  if (first) {
    const int sl = slice_of_gain_real(M, i, fpad);
    if (M.nslices > 1) st += sl;
    var = 2 * sl + (int)(i & 1);
  } else {
    const int plane = i >= ncoef ? 1 : 0;
    const int n = (int)(i - (long long)plane * ncoef);
    if (M.nslices > 1) st += slice_of_coef(M, n);
    int lo = 0, hi = ncvar - 1;  // largest k with cvar_ptr[k] <= n
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cvar_ptr[mid] <= n) lo = mid; else hi = mid - 1;
    }
    var = 2 * M.nslices + plane * ncvar + lo;
  }
  if (st->done) return;
  const T u = first ? ua[i] : ub[i];
  const T pi = S.p[i] - (T)(st->k[0] * ratio[var]) * u;
  S.p[i] = pi;
  if (st->improved) S.snap[i] = pi;
}

// ---- one launch for the whole tail of a train step (the common path: no two-adjoint-set regulariser to combine): the
// bookkeeping of finalize_kernel, the optimizer update of adam2_kernel and, for groups whose items were split, the sum
// of their partial coefficient gradients (coeff_partial_reduce_kernel) -- three launches and two kernel boundaries less per
// step, which is what a step of a small problem consists of (HERA-37 fp64: 82 -> ~69 us).
// The loop state is double-buffered: every block derives the step's decisions (stop? non-finite? bias-corrected step
// sizes, new minimum?) from the OLD state `in` and the reduced sums, and only block 0 writes the NEW state `out`, which
// the kernels of the next step read -- so no block can see a half-updated state.
template <typename T>
struct PartialSum {          // gradient of coefficient n = sum over the items q of its group of gcp[item_goff[q] + k]
  const T* gcp_r; const T* gcp_i;
  const int* coef_grp; const int* grp_coff; const int* grp_item_ptr; const int* item_goff;
  int ncoef;                 // 0: the gradient is read from AdamSet::g as it stands
};
template <typename T> struct SliceStep { StepCoef<T> c; int update, improved; };  // one slice's decisions of a step
template <typename T>
__global__ __launch_bounds__(256) void step_update_kernel(const AdamSet<T> a, const AdamSet<T> b, const PartialSum<T> ps,
                                                         const DevState* __restrict__ in, DevState* __restrict__ out,
                                                         const double* __restrict__ scal, double* __restrict__ losses, int losses_cap,
                                                         const SliceMap M, int fpad, int ncoef) {
  // ---- the step's decisions, slice by slice: threads 0 .. nslices - 1 of every block derive them (identically), block 0 records them
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  SliceStep<T>* sh = reinterpret_cast<SliceStep<T>*>(dyn_smem);  // [nslices]
  __shared__ int sh_any;
  if (threadIdx.x == 0) sh_any = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < M.nslices; t += blockDim.x) {
    DevState s = in[t];
    const bool writer = blockIdx.x == 0;
    const bool update = advance_state(s, scal[4 * t + 0], scal[4 * t + 1], scal[4 * t + 2], writer, losses + (size_t)t * losses_cap, losses_cap, true);
    if (writer) out[t] = s;
    sh[t].update = update ? 1 : 0;
    sh[t].improved = s.improved;
    sh[t].c = step_coef<T>(s);
    if (update) sh_any = 1;
  }
  __syncthreads();
  if (!sh_any) return;
  // ---- the update: sets a (gains) and b (coefficients) as one index space, grid-stride (the decisions above are taken
  // once per block, so a big problem runs a few thousand blocks, not one per 256 elements)
  const long long total = a.n + b.n;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const bool first = e < a.n;
    const AdamSet<T>& S = first ? a : b;
    const long long i = first ? e : e - a.n;
    const int sl = M.nslices > 1 ? (first ? slice_of_gain_real(M, i, fpad) : slice_of_coef_real(M, i, ncoef)) : 0;
    if (!sh[sl].update) continue;
    const StepCoef<T> c = sh[sl].c;
    const bool improved = sh[sl].improved != 0;
    T gi;
    if (!first && ps.ncoef > 0) {
      const int plane = i >= ps.ncoef ? 1 : 0;
      const int n = (int)(i - (long long)plane * ps.ncoef);
      const int g = ps.coef_grp[n];
      const int k = n - ps.grp_coff[g];
      const T* src = plane ? ps.gcp_i : ps.gcp_r;
      gi = 0;
      for (int q = ps.grp_item_ptr[g]; q < ps.grp_item_ptr[g + 1]; ++q) gi += src[ps.item_goff[q] + k];
    } else {
      gi = S.g[i];
    }
    T mi = S.m[i], vi = S.v[i];
    const T pi = optimizer_step<T>(S.p[i], gi, mi, vi, c);
    S.m[i] = mi;
    S.v[i] = vi;
    S.p[i] = pi;
    if (improved) S.snap[i] = pi;
  }
}

// ---- the WHOLE tail of a train step in one launch, for problems whose step is a few tens of microseconds (the tutorial,
// HERA-37): the per-antenna reduction of gain_grad_kernel, the loop bookkeeping of finalize_kernel, the regulariser's fold of
// combine_*_kernel and the optimizer update -- a step is then TWO launches (fused pass, tail), which cal_solver_run replays
// from a hipGraph.  Same arithmetic, operation for operation and in the same order, as the separate kernels (shared helpers
// below; bit-identical trajectories are tested), arranged so that no block depends on another:
//   * every block sums the per-item loss partials itself (the fixed order of gain_grad_kernel's last block) and derives the
//     step's decisions from the OLD state copy, as step_update_kernel does;
//   * gain blocks = (antenna, 64 CPL channels): segmented reduction over the antenna's baselines, then the update of exactly
//     those gains.  They READ the other antennas' gains while their owners update them, so the gains are double-buffered
//     (read `gains_in`, write `gains_out`; the host swaps the two after every step);
//   * the remaining blocks update the coefficients (partial gradients of split groups summed on the fly).
template <typename T>
struct TailArgs {
  const vec2_t<T>* q0; const vec2_t<T>* q1;
  const vec2_t<T>* gains_in; vec2_t<T>* gains_out;
  T* gains_m; T* gains_v; T* gains_snap;         // flat [nants][fpad][2]
  const int* ant_ptr; const int2* ant_ent;
  AdamSet<T> coef;                               // g = first gradient set; n = 0 when the model is frozen
  const T* coef_g1;                              // REG: the set that multiplies alpha (summed sets when ps1.ncoef == 0)
  PartialSum<T> ps0, ps1;
  const double* part; int nparts;
  int nants, fpad, nblk_gain;
  const DevState* in; DevState* out;             // [nslices] each
  double* losses; int losses_cap;                // [nslices][losses_cap]
  SliceMap M;
  const int* cblk_ptr;                           // several slices: [nslices + 1] the coefficient blocks of every slice (block index - nblk_gain)
  int ncoef;
};
template <typename T, bool REG>
__global__ __launch_bounds__(256) void step_tail_kernel(const TailArgs<T> A) {
  using T2 = vec2_t<T>;
  constexpr int CPL = 16 / (int)sizeof(T2) > 0 ? 16 / (int)sizeof(T2) : 1;
  typedef T vec_t __attribute__((ext_vector_type(2 * CPL)));
  __shared__ double sh[12];
  __shared__ double sh_ar, sh_ai;
  __shared__ StepCoef<T> sh_c;
  __shared__ int sh_update, sh_improved;
  __shared__ T s_part[3][3][64][2 * CPL];
  const int tid = threadIdx.x;
  const bool gain_block = (int)blockIdx.x < A.nblk_gain;
  // ---- gain block: gain_grad_kernel's reduction (antenna_sums) for (antenna a, 64 CPL channels)
  const int cb = gain_block ? blockIdx.x / A.nants : 0;
  const int a = gain_block ? blockIdx.x - cb * A.nants : 0;
  // the time slice this block works for (its loss, its loop state, its decisions), and -- coefficient blocks -- its share of it
  int slice = 0;
  long long cblk = (long long)blockIdx.x - A.nblk_gain, ncblk = (long long)gridDim.x - A.nblk_gain;  // this block among the slice's coefficient blocks
  int c0 = 0, nc = A.ncoef;  // the slice's coefficients: [c0, c0 + nc) of each plane
  if (A.M.nslices > 1) {
    if (gain_block) {
      slice = a / A.M.na_slice;
    } else {
      int lo = 0, hi = A.M.nslices - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (A.cblk_ptr[mid] <= (int)cblk) lo = mid; else hi = mid - 1;
      }
      slice = lo;
      ncblk = A.cblk_ptr[slice + 1] - A.cblk_ptr[slice];
      cblk -= A.cblk_ptr[slice];
      c0 = A.M.coff[slice];
      nc = A.M.coff[slice + 1] - c0;
    }
  }
  // A step of such a problem is a chain of dependent memory round trips, about a microsecond each, so everything that does
  // not depend on the step's decisions is requested first and the chains run side by side: the loss partials and the loop
  // state (-> decisions), and, in a gain block, antenna list -> gbar_G rows and gains (-> gradient) and the block's own gains
  // and optimizer slots.  The decisions only gate the final writes.
  double x[3];
  int p0, np;
  slice_partials(A.M, slice, A.nparts, A.part, p0, np, x);
  DevState s;
  if (tid == 0) s = A.in[slice];
  const int lane = tid & 63, seg = tid >> 6;
  const int f = (cb * 64 + lane) * CPL;
  const long long idx = (long long)a * A.fpad + f;
  T s0[2 * CPL], s1[2 * CPL], s2[2 * CPL];
  vec_t pin, mm, vv;
  bool mine = false;
  if (gain_block) {
    if (seg == 0 && f < A.fpad) {
      pin = *reinterpret_cast<const vec_t*>(A.gains_in + idx);
      mm = *reinterpret_cast<const vec_t*>(A.gains_m + 2 * idx);
      vv = *reinterpret_cast<const vec_t*>(A.gains_v + 2 * idx);
    }
    mine = antenna_sums<T, REG>(A.q0, A.q1, A.gains_in, A.ant_ptr, A.ant_ent, a, f, A.fpad, s_part, s0, s1, s2);
  }
  // ---- loss partial sums of the slice (sum_partials: the order of gain_grad_kernel's last blocks), in every block
  double tot[3];
  sum_partials(A.part, A.M.part_idx, p0, np, x, sh, tot);
  // ---- the slice's decisions of this step (advance_state): thread 0 of every block; the slice's first gain block records them
  if (tid == 0) {
    const bool writer = gain_block && cb == 0 && a == slice * A.M.na_slice;
    const bool upd = advance_state(s, tot[0], tot[1], tot[2], writer, A.losses + (size_t)slice * A.losses_cap, A.losses_cap, true);
    if (writer) A.out[slice] = s;
    sh_update = upd ? 1 : 0;
    sh_improved = s.improved;
    sh_c = step_coef<T>(s);
    sh_ar = s.alpha_r;
    sh_ai = s.alpha_i;
  }
  __syncthreads();
  const bool update = sh_update != 0;
  const StepCoef<T> sc = sh_c;
  const T ar = (T)sh_ar, ai = (T)sh_ai;
  const bool improved = sh_improved != 0;
  if (gain_block) {
    // the update of exactly these gains.  A step that does not update (loop ended, non-finite loss) still copies them to the
    // other buffer: the host swaps the buffers after every step
    if (mine) {
      vec_t pout = pin;
      if (update) {
        if (REG) {
#pragma unroll
          for (int c = 0; c < CPL; ++c) fold_gain(s0[2 * c], s0[2 * c + 1], s1[2 * c], s1[2 * c + 1], s2[2 * c], s2[2 * c + 1], ar, ai);
        }
#pragma unroll
        for (int c = 0; c < 2 * CPL; ++c) {
          T mi = mm[c], vi = vv[c];
          pout[c] = optimizer_step<T>(pin[c], s0[c], mi, vi, sc);
          mm[c] = mi;
          vv[c] = vi;
        }
        *reinterpret_cast<vec_t*>(A.gains_m + 2 * idx) = mm;
        *reinterpret_cast<vec_t*>(A.gains_v + 2 * idx) = vv;
        if (improved) *reinterpret_cast<vec_t*>(A.gains_snap + 2 * idx) = pout;
      }
      *reinterpret_cast<vec_t*>(A.gains_out + idx) = pout;
    }
    return;
  }
  // ---- coefficient blocks: element j of the slice's 2 nc reals (re plane, then im plane) = element i of the flat planes
  if (!update) return;
  const AdamSet<T>& S = A.coef;
  const long long n2 = S.n / 2;  // = ncoef: the planes are [r | i], each n2 long
  for (long long j = cblk * blockDim.x + tid; j < 2LL * nc; j += ncblk * blockDim.x) {
    const bool imag = j >= nc;
    const long long i = (imag ? n2 + (j - nc) : j) + c0;
    T gi, g1 = 0;
    if (A.ps0.ncoef > 0) {
      const int plane = imag ? 1 : 0;
      const int n = (int)(i - (long long)plane * A.ps0.ncoef);
      const int g = A.ps0.coef_grp[n];
      const int k = n - A.ps0.grp_coff[g];
      const T* src = plane ? A.ps0.gcp_i : A.ps0.gcp_r;
      gi = 0;
      for (int q = A.ps0.grp_item_ptr[g]; q < A.ps0.grp_item_ptr[g + 1]; ++q) gi += src[A.ps0.item_goff[q] + k];
      if (REG) {
        const T* src1 = plane ? A.ps1.gcp_i : A.ps1.gcp_r;
        for (int q = A.ps0.grp_item_ptr[g]; q < A.ps0.grp_item_ptr[g + 1]; ++q) g1 += src1[A.ps0.item_goff[q] + k];
      }
    } else {
      gi = S.g[i];
      if (REG) g1 = A.coef_g1[i];
    }
    if (REG) {
      // combine_coeff_kernel: g0_r += ar g1_r - ai g1_i ; g0_i += ar g1_i + ai g1_r
      const long long jo = imag ? i - n2 : i + n2;  // the same coefficient's other plane
      T o1;
      if (A.ps0.ncoef > 0) {
        const int plane = imag ? 0 : 1;
        const int n = (int)(jo - (long long)plane * A.ps0.ncoef);
        const int g = A.ps0.coef_grp[n];
        const int k = n - A.ps0.grp_coff[g];
        const T* src1 = plane ? A.ps1.gcp_i : A.ps1.gcp_r;
        o1 = 0;
        for (int q = A.ps0.grp_item_ptr[g]; q < A.ps0.grp_item_ptr[g + 1]; ++q) o1 += src1[A.ps0.item_goff[q] + k];
      } else {
        o1 = A.coef_g1[jo];
      }
      gi = fold_coeff(gi, g1, o1, ar, ai, imag);
    }
    T mi = S.m[i], vi = S.v[i];
    const T pi = optimizer_step<T>(S.p[i], gi, mi, vi, sc);
    S.m[i] = mi;
    S.v[i] = vi;
    S.p[i] = pi;
    if (improved) S.snap[i] = pi;
  }
}

// ---- the reference's graph functions under their own names (not on the fit's path, which never materialises a model) -------
// data_model (calibration.py:1593-1605) on top of MODE_MODEL's A c: m <- g_ant0 conj(g_ant1) m, in place, [nbls][fpad]
template <typename T>
__global__ void apply_gains_kernel(T* __restrict__ m_r, T* __restrict__ m_i, const vec2_t<T>* __restrict__ gains, const int2* __restrict__ bl_ant,
                                   long long nbls, int fpad) {
#pragma clang fp contract(off)
  const long long total = nbls * fpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / fpad;
    const int f = (int)(i - b * fpad);
    const int2 ant = bl_ant[b];
    const vec2_t<T> g0 = gains[(long long)ant.x * fpad + f], g1 = gains[(long long)ant.y * fpad + f];
    const T gr = g0.x * g1.x + g0.y * g1.y, gi = g0.y * g1.x - g0.x * g1.y;  // g0 conj(g1), split as in :1599-1602
    const T vr = m_r[i], vi = m_i[i];
    m_r[i] = gr * vr - gi * vi;
    m_i[i] = gr * vi + gi * vr;
  }
}
// mse (calibration.py:1608-1609): per-block partial sums (double, fixed order) of w ((d_r - m_r)^2 + (d_i - m_i)^2); a second launch
// with one block adds the partials
template <typename T>
__global__ __launch_bounds__(256) void square_error_kernel(const T* __restrict__ m_r, const T* __restrict__ m_i, const T* __restrict__ d_r,
                                                           const T* __restrict__ d_i, const T* __restrict__ w, long long n, double* __restrict__ part) {
#pragma clang fp contract(off)
  double acc = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const T er = d_r[i] - m_r[i], ei = d_i[i] - m_i[i];
    acc += (double)((er * er + ei * ei) * w[i]);
  }
  __shared__ double sh[4];
  acc = ldsum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
  __shared__ double sh[4];
  acc = ldsum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ---- setup kernels -------------------------------------------------------------------------------------------
template <typename T>
__global__ void fill_kernel(T* __restrict__ dst, long long n, T value) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = value;
}

// unique basis block (row-major [nrb * nfreqs][nvec]) -> tile-major [rowblk][channel block][vec][FB], zero padded
template <typename T>
__global__ void retile_kernel(const T* __restrict__ src, T* __restrict__ dst, int nfreqs, int fpad, int nvec, int nrb, int fb) {
  const long long total = (long long)nrb * fpad * nvec;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int fl = (int)(i % fb);
    long long r = i / fb;
    const int k = (int)(r % nvec);
    r /= nvec;
    const int ntpb = fpad / fb;
    const int fbk = (int)(r % ntpb);
    const int rb = (int)(r / ntpb);
    const int f = fbk * fb + fl;
    dst[i] = f < nfreqs ? src[((long long)rb * nfreqs + f) * nvec + k] : (T)0;
  }
}

struct CopyJob { long long src, dst, n; };  // element offsets / count (multiples of 16 B)
template <typename T>
__global__ void tile_copy_kernel(const T* __restrict__ src, T* __restrict__ dst, const CopyJob* __restrict__ jobs) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T v_t __attribute__((ext_vector_type(16 / sizeof(T))));
  const CopyJob j = jobs[blockIdx.x];
  const v_t* s = reinterpret_cast<const v_t*>(src + j.src);
  v_t* d = reinterpret_cast<v_t*>(dst + j.dst);
  for (long long i = threadIdx.x; i < j.n / VEC; i += blockDim.x) d[i] = s[i];
}

// [rows][nfreqs] host layout <-> [rows][fpad] device layout (zero padded), optionally interleaving (re, im)
template <typename T>
__global__ void pad_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, long long rows, int nfreqs, int fpad, int dst_stride,
                                int dst_off) {
  const long long total = rows * fpad;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / fpad;
    const int f = (int)(i - r * fpad);
    dst[i * dst_stride + dst_off] = f < nfreqs ? src[r * nfreqs + f] : (T)0;
  }
}
template <typename T>
__global__ void unpad_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, long long rows, int nfreqs, int fpad, int src_stride,
                                  int src_off) {
  const long long total = rows * nfreqs;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / nfreqs;
    const int f = (int)(i - r * nfreqs);
    dst[i] = src[(r * fpad + f) * src_stride + src_off];
  }
}

}  // namespace calk
