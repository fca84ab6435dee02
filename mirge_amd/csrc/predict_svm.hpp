// Predict mode's classification (reference utils/preprocess_featureFiles.py and utils/model_predict.py): the RBF SVM of
// the model file on the device (predict_svm.hip, behind mrg_predict_svm in capi.hip) and the host side around it
// (predict_model_write.cpp: the three filter files, the feature matrix, the two result files).  The rule:
// tests/predict_model_model.py.  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace mrg {

constexpr uint32_t kSvmMaxFeatures = 64;  // a row's standardised features stay in registers
constexpr uint32_t kSvmTile = 64;         // support vectors staged through LDS at a time
constexpr uint32_t kSvmBlock = 64;        // rows of a workgroup: one wave, one row a lane
static_assert(kSvmBlock == kSvmTile, "a lane stages one coefficient and NFP elements of a tile: lanes and tile rows must be equally many");

struct SvmModelDev {   // the model's arrays on the device, float64
  uint32_t nf, n_sv;
  const double* mean;    // [nf]
  const double* scale;   // [nf]
  const double* sv;      // [n_sv][nf], standardised
  const double* coef;    // [n_sv]
  double intercept, gamma, prob_a, prob_b;
};

// One lane per row: pred [n] = 1 or -1, dec [n], prob [n][2] (class -1, class 1).  Nothing is launched for n_rows = 0.
hipError_t predict_svm_launch(uint64_t n_rows, const double* x, const SvmModelDev& m, int8_t* pred, double* dec, double* prob,
                              hipStream_t stream);

// predict_model_write.cpp (host, no GPU).  Throw std::invalid_argument (input that contradicts itself) or std::runtime_error.
struct ModelTable {
  uint64_t n_table = 0, n_dataset = 0, n_refined = 0;  // lines below the header: the table's, the first filter's, the second's
  uint32_t nf = 0;
  uint32_t n_stray = 0;           // selected names whose column holds a cell that is no number: 0 for every row
  std::string header3;            // the three leading column names, joined by commas
  std::vector<std::string> names; // [n_refined] the three leading cells of every row, joined by commas
  std::vector<double> x;          // [n_refined][nf] raw feature rows
};
struct ModelFilterArgs {
  const char* table_path;
  const char* dataset_path;
  const char* refined_tmp_path;
  const char* refined_path;
  const char* namelist;   // the namelist's names, one a line
  const char* features;   // the model's selected names in its order, one a line
};
void filter_model_table(const ModelFilterArgs& a, ModelTable* out);
// the two result files from pred [n_refined] and prob [n_refined][2]; counts the rows predicted 1 and the rows kept
void write_model_results(const ModelTable& t, const int8_t* pred, const double* prob, const char* detailed_path, const char* novel_path,
                         uint64_t* predicted, uint64_t* kept);
// Python's repr of a finite double appended to out
void append_repr(std::string& out, double v);

}  // namespace mrg
