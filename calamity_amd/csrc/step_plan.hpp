// step_plan.hpp -- the shape of one pass or train step: which kernels follow the fused / dense pass, which form the update takes and
// whether the steps are replayed from a graph, decided once on the host from what set-up and the setters left behind.  Plain
// arithmetic: no HIP or RCCL call and no solver.  SolverT::step_shape fills the inputs; enqueue_pass, enqueue_step and run read the
// result and derive no condition of their own.  cal_debug_step_shape returns it without a device (tests/test_step_plan_host.py).
#pragma once
#include "../../include/calamity_hip.h"

namespace {

constexpr int kGraphSteps = 16;      // steps per replay of the two-launch step; even: the double-buffered loop state and gains end a replay where they began
constexpr int kGraphStepsLarge = 8;  // ... of a large problem's kernel-by-kernel step
// capturing and instantiating the graph of a large problem's steps costs tens of milliseconds -- 40 for 16 steps of the dense path --,
// once per shape of call: calls of fewer steps launch kernel by kernel, longer ones replay kGraphStepsLarge steps at a time
constexpr int kGraphMinSteps = 256;

// what a pass is asked for
struct PassAsk {
  bool grads;         // gradients, not the loss alone
  bool apply_update;  // a train step: loop bookkeeping and the update follow
  bool project;       // the gain-gradient planes are projected on the gain basis BEFORE the exchange (the pass serves y)
};
constexpr PassAsk kLossPass{false, false, false};
constexpr PassAsk kGradPass{true, false, false};
constexpr PassAsk kProjectedGradPass{true, false, true};
constexpr PassAsk train_step(bool gain_basis) { return PassAsk{true, true, gain_basis}; }

struct StepInputs {     // (cal_debug_step_shape takes them in this order, one int32 each)
  bool dense;           // the dense (matrix-core) kernels serve the pass: mf_ok
  bool reg_sum;         // the regulariser is "sum"
  bool reg_prepass;     // baselines that share tiles need every slice's alpha before their gradient pass (set_problem; agreed over the ranks)
  bool gc_direct;       // every group is one item: the kernels write the coefficient gradient itself
  bool comm;            // a communicator or an exchange hook is set
  bool gain_basis;      // the optimizer's gain variables are y: a frequency basis, a time basis or both
  bool small;           // 2 nants fpad + 2 ncoef <= 2^20 reals
  int launch_mode;      // cal_launch_mode
  bool lamb;            // the optimizer is LAMB
  PassAsk ask;
  bool timing;          // (the replay rule only) HIP events around every pass
  bool long_run;        // (the replay rule only) nsteps >= kGraphMinSteps
};

// no train step; step_tail_kernel: everything behind the fused pass; step_update_kernel: loop bookkeeping + update (+ the partial
// coefficient-gradient sums); behind finalize_kernel LAMB's four launches; behind finalize_kernel adam2_kernel
enum UpdateForm : int { UPDATE_NONE = 0, UPDATE_TAIL = 1, UPDATE_FUSED = 2, UPDATE_LAMB = 3, UPDATE_ADAM2 = 4 };

struct StepShape {      // (cal_debug_step_shape returns the fields from Rk on in this order, one int32 each)
  bool dense, reg, grads;  // carried through from the inputs for the launchers
  bool Rk;              // the general kernel's two-adjoint-set form of the regulariser: a second gradient set, the combine kernels
  bool two_pass;        // dense path + regulariser: a loss-only pass yields S (hence alpha = 2 (S - P)), then the gradient pass applies
                        // e = -2 w r + alpha w directly -- no second adjoint set, no combine kernels
  bool prepass;         // general path: loss pass, the slices' sums and alpha before the gradient pass (the multi-slice kernels have no second adjoint set)
  bool tail1;           // step_tail_kernel follows the fused pass at once
  bool fused_update;    // step_update_kernel
  bool partial_reduce;  // coeff_partial_reduce_kernel (a second one where Rk)
  bool finalize;        // finalize_kernel
  int planes;           // gain-gradient planes that are projected, exchanged and combined: 3 where Rk, else 1
  bool proj;            // the planes are projected on the gain basis
  int update;           // UpdateForm
  bool expand;          // the gains are rebuilt from y behind the update
  bool replay;          // the steps of a run are replayed from a graph
  bool partials;        // the pass leaves the coefficient gradient as per-item partials: whoever consumes it sums them
};
constexpr int kStepShape = 13;

inline StepShape plan_step(const StepInputs& in) {
  StepShape s{in.dense, in.reg_sum, in.ask.grads};
  const bool train = in.ask.grads && in.ask.apply_update;
  s.Rk = in.reg_sum && !in.dense;
  s.two_pass = in.dense && in.reg_sum && in.ask.grads;
  s.prepass = !in.dense && in.ask.grads && in.reg_sum && in.reg_prepass;
  s.partials = !in.gc_direct && !in.dense;
  // Small problems (a step of tens of microseconds: HERA-37, the tutorial) gain from one launch instead of three for the
  // tail of a step; with millions of parameters the per-block decision prologue of the fused kernel costs more than the two
  // kernel boundaries it saves (HERA-350: 105 us against 5 + 56 us), so those keep finalize_kernel + adam2_kernel.
  // (CAL_LAUNCH_KERNELS keeps every kernel its own launch: finalize_kernel + adam2_kernel at any size)
  // (... and LAMB's update is four launches of its own: per-variable norms sit between the moments and the parameters)
  const bool fits = in.small && in.launch_mode != CAL_LAUNCH_KERNELS && !in.lamb;
  // Problems whose step is tens of microseconds: the whole tail as ONE launch (step_tail_kernel) -- no communicator (the
  // exchange sits between the reduction and the update), general kernels, and not when every kernel is asked to be its own launch
  // (... nor with the regulariser over baselines that share tiles: alpha is needed between that path's two passes)
  // (... nor with a gain basis: the projection sits between the antenna reduction and the update, which step_tail_kernel fuses)
  s.tail1 = train && !in.comm && !in.dense && !in.gain_basis && fits && !(in.reg_sum && in.reg_prepass);
  // everything below sits behind the pass: with the one-launch tail none of it is a launch of its own
  s.fused_update = !s.tail1 && in.ask.apply_update && !s.Rk && fits;
  s.partial_reduce = !s.tail1 && in.ask.grads && s.partials && !s.fused_update;
  s.finalize = !s.tail1 && !s.fused_update;
  s.planes = s.Rk ? 3 : 1;
  s.proj = !s.tail1 && in.ask.project && in.ask.grads;
  // (LAMB is refused while a basis is set -- set_optimizer, set_gain_basis --: with y as the gain set the update is never LAMB's)
  s.update = !in.ask.apply_update ? UPDATE_NONE : s.tail1 ? UPDATE_TAIL : s.fused_update ? UPDATE_FUSED : (in.lamb && !in.gain_basis) ? UPDATE_LAMB : UPDATE_ADAM2;
  s.expand = in.ask.apply_update && !s.tail1 && in.gain_basis;
  // hipGraph replay of kGraphSteps train steps at a time: the steps of such problems are bound by launch latency.  Timed
  // runs (HIP events around every fused pass) issue their launches one by one.
  // Large problems replay too unless the step holds an exchange (a collective or a host callback is not captured).
  // Of the large problems only the dense path replays in "auto": measured at HERA-350 (tools/graph_ab.py) its step is the same or 0.5 % shorter
  // from a graph, the streaming kernel's step 3-13 % LONGER (4.9 -> 5.1, 4.7 -> 5.3 ms on two boxes: what the passes leave in the caches
  // for the kernels behind them does not survive the graph's node boundaries).
  s.replay = train && (s.tail1 || (!in.comm && ((in.dense && in.long_run) || in.launch_mode == CAL_LAUNCH_GRAPH))) && !in.timing &&
             (in.launch_mode == CAL_LAUNCH_AUTO || in.launch_mode == CAL_LAUNCH_GRAPH);
  return s;
}

// the two layouts of cal_debug_step_shape
inline StepInputs step_inputs_from(const int32_t* v) {
  return {v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7], v[8] != 0, {v[9] != 0, v[10] != 0, v[11] != 0}, v[12] != 0, v[13] != 0};
}
inline void step_shape_to(const StepShape& s, int32_t* o) {
  const int32_t v[kStepShape] = {s.Rk, s.two_pass, s.prepass, s.tail1, s.fused_update, s.partial_reduce, s.finalize, s.planes, s.proj, s.update, s.expand, s.replay, s.partials};
  for (int i = 0; i < kStepShape; ++i) o[i] = v[i];
}

}  // namespace
