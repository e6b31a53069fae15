// ob_builder.hpp -- the builder's handles (ob_builder.cpp), for the front ends that extend a prepared run
// (ob_jackknife.cpp): the configuration, the prepared run, the results.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ob_engine.hpp"
#include "ob_frame.hpp"
#include "ob_dr.hpp"
#include "ob_jackknife.hpp"

namespace ob {

struct Config {
  std::string outcome, group, reference_group;
  std::vector<std::string> outcomes;  // RIF multi-tau: y columns of one panel (empty: {outcome})
  std::vector<std::string> predictors, categorical, normalize;
  bool has_weights = false;
  std::string weights;
  bool has_selection = false;
  std::string selection;
  std::vector<std::string> selection_predictors;
  uint64_t reps = 20;
  int ref = OB_REF_GROUP_A;
  bool has_seed = false;
  uint64_t seed = 0;
  // cluster bootstrap (ob_cluster.hpp): the id column and the sampling mode
  bool has_cluster = false;
  std::string cluster;
  bool cluster_stratified = false;
};

struct ClusterState;

}  // namespace ob

struct ob_results {
  double total_gap = 0.0;
  int64_t n_a = 0, n_b = 0, n_failed = 0;
  int64_t n_clusters = -1;  // a clustered run's C (ob_results_n_clusters), else -1
  struct Comp {
    std::string name;
    double estimate, std_err, t_stat, p_value, ci_lower, ci_upper;
    double jack[5] = {NAN, NAN, NAN, NAN, NAN};  // ob_results_jackknife: accel, jack_se, jack_bias, z0, flag
  };
  std::vector<Comp> tables[5];
  bool has_jack = false;  // ob_prepared_finish_bca / ob_builder_run_bca filled Comp::jack
  std::vector<double> residuals, xa_mean, xb_mean, beta_star;
};

struct ob_prepared {
  ob_ctx* ctx = nullptr;
  ob_panel* panel = nullptr;
  ob::Config cfg;
  int ref = OB_REF_GROUP_A;
  uint64_t seed = 0;
  int k = 0, n_base = 0, row_len = 0;
  std::vector<std::string> names;         // K final predictor names
  std::vector<std::string> detail_names;  // K + n_base (base categories appended)
  std::vector<double> point_row, resid_b;  // n_y x row_len, n_y x n_b
  int64_t n_a = 0, n_b = 0;
  int n_y = 1;
  int64_t n_resid = 0;                     // residuals per outcome: n_b, or B's selected rows (Heckman)
  std::vector<std::string> selection_names;  // Heckman: intercept + selection predictors
  // ob_prepared_jackknife: the pass's result and its [C][3] statistics, kept for ob_prepared_finish_bca
  ob::JackResult jack;
  std::vector<double> jack_stats;
  bool has_jack = false;
  // ob_builder_prepare_clustered: the cluster index and Q on the device; boots run through ob_cluster.hip
  ob::ClusterState* cluster = nullptr;
  // a model front end's handle (ob_model.hpp): its ob::ModelKind and its state on the device; boots run through the
  // kind's hooks
  int model_kind = 0;
  void* model = nullptr;
  // ob_builder_prepare_dr: the thresholds, quantiles and point fits on the host
  ob::DrInfo dr_info;
};

namespace ob {

int config_from(const ob_builder_config* c, Config& out);
// clean_dataframe -> dummies -> split -> prepare_data -> upload -> point estimate (builder.rs:787-814)
int prepare(ob_ctx* ctx, const Frame& input, const Config& c, ob_prepared** out);
// builder.rs:841-950 over successful rows in replicate order, for outcome t (rows/ok: its block)
int finish(const ob_prepared* pr, int t_out, const double* rows, const uint8_t* ok, uint64_t n_reps, ob_results** out);
// ob_jackknife.cpp: finish(), then every component's interval through bca_stats with the accelerations of
// pr->jack_stats ([C][3], filled by a jackknife pass over the handle)
int finish_bca(const ob_prepared* pr, const double* rows, const uint8_t* ok, uint64_t n_reps, double level,
               ob_results** out);
// ob_builder_data_matrices, with the groups' sample weights kept where want_w (matrices_weights: NULL without
// a weights column; the weight column's dtype and sign are checked as prepare() checks them)
int data_matrices(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, bool want_w,
                  ob_matrices** out);
const double* matrices_weights(const ob_matrices* m, int g);

}  // namespace ob
