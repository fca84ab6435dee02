// Predict mode's classifier on the device: sklearn's SVC.predict and predict_proba for the two-class RBF model of a miRge2.0
// model file, as libsvm computes them (svm_predict_values, sigmoid_predict, multiclass_probability), from raw feature rows.
// The rule: tests/predict_model_model.py.
//
// One lane per row, one wave per workgroup.  A lane standardises its row into registers and adds the terms
//     coef_i * exp(-gamma * sum_j (z_j - sv_ij)^2)
// one support vector after the other in their stored order, the intercept last: a row's result depends on nothing but the
// row, neither on its place in the batch nor on the launch geometry, and there is no atomic.  The support vectors are NOT
// split over waves, so there are no partial sums to combine: at the 10^3 to 10^5 rows predict mode has, the launch underfills
// the device and is bound by the latency of one lane's chain (n_sv exps), which is milliseconds at most.
//
// The support vectors come through LDS in tiles of kSvmTile, each row padded to NFP = nf rounded up to 8 with zeros (a padded
// feature adds (0 - 0)^2 = +0 to a sum that is not negative: nothing).  Every lane reads the same element of the tile at a
// time: a broadcast.  The next tile is fetched into registers while the current one is worked on.  All arithmetic is float64
// with contraction off: products and sums round one by one as libsvm's do on the host, and the squared distance has the
// (z - sv)^2 form (|z|^2 + |sv|^2 - 2 z.sv rounds differently).
#include "predict_svm.hpp"

namespace mrg {

#pragma clang fp contract(off)

namespace {

// libsvm's sigmoid_predict
__device__ inline double svm_sigmoid(double f, double a, double b) {
  const double v = f * a + b;
  if (v >= 0) {
    const double e = exp(-v);
    return e / (1.0 + e);
  }
  return 1.0 / (1.0 + exp(v));
}

// libsvm's multiclass_probability for k = 2 from r01 = the pairwise probability of the first class: p starts at 1/2, the
// iteration stops below eps = 0.005 / 2 or after 100 rounds
__device__ inline void svm_couple(double r01, double* p0, double* p1) {
  const double r10 = 1.0 - r01;
  const double q[2][2] = {{r10 * r10, -r10 * r01}, {-r10 * r01, r01 * r01}};
  double p[2] = {0.5, 0.5};
  const double eps = 0.005 / 2;
  for (int iter = 0; iter < 100; ++iter) {
    double qp[2] = {q[0][0] * p[0] + q[0][1] * p[1], q[1][0] * p[0] + q[1][1] * p[1]};
    double pqp = p[0] * qp[0] + p[1] * qp[1];
    const double e0 = fabs(qp[0] - pqp), e1 = fabs(qp[1] - pqp);
    if ((e1 > e0 ? e1 : e0) < eps) break;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const double diff = (-qp[t] + pqp) / q[t][t];
      p[t] += diff;
      pqp = (pqp + diff * (diff * q[t][t] + 2 * qp[t])) / (1 + diff) / (1 + diff);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        qp[j] = (qp[j] + diff * q[t][j]) / (1 + diff);
        p[j] /= (1 + diff);
      }
    }
  }
  *p0 = p[0];
  *p1 = p[1];
}

template <int NFP>
__global__ __launch_bounds__(kSvmBlock) void predict_svm_kernel(uint64_t n_rows, const double* __restrict__ x, SvmModelDev m,
                                                                int8_t* __restrict__ pred, double* __restrict__ dec,
                                                                double* __restrict__ prob) {
  __shared__ double tile[kSvmTile * NFP];
  __shared__ double tile_coef[kSvmTile];
  const uint32_t lane = threadIdx.x;
  const uint64_t row = (uint64_t)blockIdx.x * kSvmBlock + lane;
  const bool live = row < n_rows;
  const uint32_t nf = m.nf, n_sv = m.n_sv;

  double z[NFP];
#pragma unroll
  for (int j = 0; j < NFP; ++j) z[j] = (live && (uint32_t)j < nf) ? (x[row * nf + j] - m.mean[j]) / m.scale[j] : 0.0;

  // element e = k * kSvmBlock + lane of the padded tile [kSvmTile][NFP] that starts at support vector t0
  double pre[NFP], pre_coef;
  auto fetch = [&](uint32_t t0) {
#pragma unroll
    for (int k = 0; k < NFP; ++k) {
      const uint32_t e = (uint32_t)k * kSvmBlock + lane, s = t0 + e / NFP, j = e % NFP;
      pre[k] = (s < n_sv && j < nf) ? m.sv[(uint64_t)s * nf + j] : 0.0;
    }
    pre_coef = t0 + lane < n_sv ? m.coef[t0 + lane] : 0.0;
  };
  fetch(0);

  double sum = 0.0;
  for (uint32_t t0 = 0; t0 < n_sv; t0 += kSvmTile) {
    __syncthreads();  // the tile before this one has been read by every lane
#pragma unroll
    for (int k = 0; k < NFP; ++k) tile[(uint32_t)k * kSvmBlock + lane] = pre[k];
    tile_coef[lane] = pre_coef;
    __syncthreads();
    if (t0 + kSvmTile < n_sv) fetch(t0 + kSvmTile);
    const uint32_t count = n_sv - t0 < kSvmTile ? n_sv - t0 : kSvmTile;
    for (uint32_t s = 0; s < count; ++s) {
      const double* v = tile + s * NFP;
      double dist = 0.0;
#pragma unroll
      for (int j = 0; j < NFP; ++j) {
        const double d = z[j] - v[j];
        dist = dist + d * d;
      }
      sum = sum + tile_coef[s] * exp(-m.gamma * dist);
    }
  }
  if (!live) return;
  const double f = sum + m.intercept;
  dec[row] = f;
  pred[row] = f < 0 ? (int8_t)-1 : (int8_t)1;
  // libsvm's own decision value is sklearn's negated, and its first class is -1
  const double min_prob = 1e-7;
  double r = svm_sigmoid(-f, m.prob_a, m.prob_b);
  r = fmin(fmax(r, min_prob), 1.0 - min_prob);
  double p0, p1;
  svm_couple(r, &p0, &p1);
  prob[2 * row] = p0;
  prob[2 * row + 1] = p1;
}

template <int NFP>
hipError_t launch(uint64_t n_rows, const double* x, const SvmModelDev& m, int8_t* pred, double* dec, double* prob, hipStream_t stream) {
  const uint32_t grid = (uint32_t)((n_rows + kSvmBlock - 1) / kSvmBlock);
  hipLaunchKernelGGL(predict_svm_kernel<NFP>, dim3(grid), dim3(kSvmBlock), 0, stream, n_rows, x, m, pred, dec, prob);
  return hipGetLastError();
}

}  // namespace

hipError_t predict_svm_launch(uint64_t n_rows, const double* x, const SvmModelDev& m, int8_t* pred, double* dec, double* prob,
                              hipStream_t stream) {
  if (n_rows == 0) return hipSuccess;
  if (m.nf < 1 || m.nf > kSvmMaxFeatures || m.n_sv < 1 || n_rows > 0x7fffffffull) return hipErrorInvalidValue;
  switch ((m.nf + 7) / 8) {
    case 1: return launch<8>(n_rows, x, m, pred, dec, prob, stream);
    case 2: return launch<16>(n_rows, x, m, pred, dec, prob, stream);
    case 3: return launch<24>(n_rows, x, m, pred, dec, prob, stream);
    case 4: return launch<32>(n_rows, x, m, pred, dec, prob, stream);
    case 5: return launch<40>(n_rows, x, m, pred, dec, prob, stream);
    case 6: return launch<48>(n_rows, x, m, pred, dec, prob, stream);
    case 7: return launch<56>(n_rows, x, m, pred, dec, prob, stream);
    default: return launch<64>(n_rows, x, m, pred, dec, prob, stream);
  }
}

}  // namespace mrg
