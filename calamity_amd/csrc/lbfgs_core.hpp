// lbfgs_core.hpp -- the two-loop recursion of L-BFGS on coefficients (the "vector-free" form): with p stored pairs the direction lies in
// the span of b = [s_1 .. s_p, y_1 .. y_p, g] (oldest pair first), so the recursion needs only the Gram matrix B[i][j] = b_i . b_j and
// works on 2p + 1 numbers instead of on vectors.  Plain arithmetic, host and device: lbfgs_coeff_kernel and lbfgs_armijo_kernel run it
// per slice, cal_debug_lbfgs_coefficients hands the same function to the tests without a device (tests/test_lbfgs_host.py).
#pragma once

namespace calk {

constexpr int kLbfgsMaxHistory = 16;                       // the cap on cal_lbfgs_desc::history
constexpr int kLbfgsMaxBasis = 2 * kLbfgsMaxHistory + 1;   // vectors the direction is a combination of

// B[i][j] = gram[idx[i] * ld + idx[j]] over b = [s_1 .. s_p, y_1 .. y_p, g]: the caller's matrix may hold the vectors in any order (the
// device keeps them by ring slot).  delta [2p + 1]: d = sum_j delta_j b_j = -H g with H the L-BFGS inverse Hessian whose initial matrix is
// gamma I, gamma = s_p . y_p / y_p . y_p.  alpha [p]: work space (the caller's, so that the device keeps it out of scratch memory).
// Returns the slope g . d.  p = 0: d = -g.
__host__ __device__ inline double lbfgs_two_loop(int p, const double* gram, int ld, const int* idx, double* delta, double* alpha) {
  const int n = 2 * p + 1;
  for (int j = 0; j < n; ++j) delta[j] = 0.0;
  delta[2 * p] = -1.0;
  for (int i = p - 1; i >= 0; --i) {
    double a = 0.0;  // (the vector so far) . s_i
    for (int j = 0; j < n; ++j) a += delta[j] * gram[idx[j] * ld + idx[i]];
    a /= gram[idx[i] * ld + idx[p + i]];  // s_i . y_i
    alpha[i] = a;
    delta[p + i] -= a;
  }
  if (p > 0) {
    const double gamma = gram[idx[p - 1] * ld + idx[2 * p - 1]] / gram[idx[2 * p - 1] * ld + idx[2 * p - 1]];
    for (int j = 0; j < n; ++j) delta[j] *= gamma;
  }
  for (int i = 0; i < p; ++i) {
    double b = 0.0;  // (the vector so far) . y_i
    for (int j = 0; j < n; ++j) b += delta[j] * gram[idx[j] * ld + idx[p + i]];
    b /= gram[idx[i] * ld + idx[p + i]];
    delta[i] += alpha[i] - b;
  }
  double slope = 0.0;
  for (int j = 0; j < n; ++j) slope += delta[j] * gram[idx[j] * ld + idx[2 * p]];
  return slope;
}

}  // namespace calk
