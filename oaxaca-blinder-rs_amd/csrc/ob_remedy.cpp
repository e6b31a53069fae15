// ob_remedy.cpp -- host side and C ABI of the pay-equity remediation: the fair-wage model, the
// prediction-interval z and the array entry points of `optimize_inner` (engine/src/analysis.rs:309-869).
//
// The engine's "A" is the reference group and "B" the target (analysis.rs:409). The fair-wage model is
// fit on A (OptimizationTarget::Reference) or on A stacked over B (Pooled) (:434-460); the covariance
// (X_A'X_A)^-1 is A's alone in both modes (:495-500). The normal equations are rows and columns of the
// extended Gram over [features, y, 1] that ob_vif.hip forms, reordered to the design's order (the
// intercept first).
//
// Deliberate difference: beta is the Cholesky solve of the normal equations in nalgebra's operation
// order (ob_linalg.hpp), not the reference's SVD solve. The reference inverts X_A'X_A two lines later and
// fails when it is singular, so the two differ by rounding of order cond u only.
//
// Also here: check_defensibility_inner (engine/src/defensibility.rs) as ob_remedy_defend / ob_remedy_defend_rows
// and verify_inner (analysis.rs:40-96) as ob_remedy_verify. Predictor overrides are resolved on the host
// (resolve_overrides) and applied to copies of the touched columns BEFORE the design is built, so an override of
// a reference-group row changes beta, cov and sigma squared for every row, as in the reference. Deliberate
// differences: a null or non-finite value in a named column is OB_E_INVALID (ob_remedy_run's checks, shared);
// the group sums are added in a fixed order (the reference's follow HashMap iteration); an adjustment whose
// index is outside the frame is skipped by ob_remedy_defend, as there, but rejected by ob_remedy_defend_rows
// and ob_remedy_verify.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include <map>
#include <set>
#include <string>

#include "ob_common.hpp"
#include "ob_frame.hpp"
#include "ob_hip.hpp"
#include "ob_linalg.hpp"
#include "ob_remedy.hpp"
#include "ob_vif.hpp"

namespace ob {

namespace {

// statrs function::evaluate::polynomial: Horner from the highest coefficient down.
template <int N>
inline double polynomial(double z, const double (&c)[N]) {
  double sum = c[N - 1];
  for (int i = N - 2; i >= 0; --i) sum = c[i] + z * sum;
  return sum;
}

// statrs function::erf: the coefficient tables of erf_inv_impl (the rational approximations of
// Boost.Math's erf_inv), numerator then denominator for each of its seven ranges.
const double kAN[] = {-0.000508781949658280665617, -0.00836874819741736770379, 0.0334806625409744615033,
                      -0.0126926147662974029034,   -0.0365637971411762664006,  0.0219878681111168899165,
                      0.00822687874676915743155,   -0.00538772965071242932965};
const double kAD[] = {1.0,
                      -0.970005043303290640362,
                      -1.56574558234175846809,
                      1.56221558398423026363,
                      0.662328840472002992063,
                      -0.71228902341542847553,
                      -0.0527396382340099713954,
                      0.0795283687341571680018,
                      -0.00233393759374190016776,
                      0.000886216390456424707504};
const double kBN[] = {-0.202433508355938759655, 0.105264680699391713268, 8.37050328343119927838,
                      17.6447298408374015486,   -18.8510648058714251895, -44.6382324441786960818,
                      17.445385985570866523,    21.1294655448340526258,  -3.67192254707729348546};
const double kBD[] = {1.0,
                      6.24264124854247537712,
                      3.9713437953343869095,
                      -28.6608180499800029974,
                      -20.1432634680485188801,
                      48.5609213108739935468,
                      10.8268667355460159008,
                      -22.6436933413139721736,
                      1.72114765761200282724};
const double kCN[] = {-0.131102781679951906451,    -0.163794047193317060787,   0.117030156341995252019,
                      0.387079738972604337464,     0.337785538912035898924,    0.142869534408157156766,
                      0.0290157910005329060432,    0.00214558995388805277169,  -0.679465575181126350155e-6,
                      0.285225331782217055858e-7,  -0.681149956853776992068e-9};
const double kCD[] = {1.0,
                      3.46625407242567245975,
                      5.38168345707006855425,
                      4.77846592945843778382,
                      2.59301921623620271374,
                      0.848854343457902036425,
                      0.152264338295331783612,
                      0.01105924229346489121};
const double kDN[] = {-0.0350353787183177984712,   -0.00222426529213447927281, 0.0185573306514231072324,
                      0.00950804701325919603619,   0.00187123492819559223345,  0.000157544617424960554631,
                      0.460469890584317994083e-5,  -0.230404776911882601748e-9, 0.266339227425782031962e-11};
const double kDD[] = {1.0,
                      1.3653349817554063097,
                      0.762059164553623404043,
                      0.220091105764131249824,
                      0.0341589143670947727934,
                      0.00263861676657015992959,
                      0.764675292302794483503e-4};
const double kEN[] = {-0.0167431005076633737133,   -0.00112951438745580278863,  0.00105628862152492910091,
                      0.000209386317487588078668,  0.149624783758342370182e-4,  0.449696789927706453732e-6,
                      0.462596163522878599135e-8,  -0.281128735628831791805e-13, 0.99055709973310326855e-16};
const double kED[] = {1.0,
                      0.591429344886417493481,
                      0.138151865749083321638,
                      0.0160746087093676504695,
                      0.000964011807005165528527,
                      0.275335474764726041141e-4,
                      0.282243172016108031869e-6};
const double kFN[] = {-0.0024978212791898131227,   -0.779190719229053954292e-5, 0.254723037413027451751e-4,
                      0.162397777342510920873e-5,  0.396341011304801168516e-7,  0.411632831190944208473e-9,
                      0.145596286718675035587e-11, -0.116765012397184275695e-17};
const double kFD[] = {1.0,
                      0.207123112214422517181,
                      0.0169410838120975906478,
                      0.000690538265622684595676,
                      0.145007359818232637924e-4,
                      0.144437756628144157666e-6,
                      0.509761276599778486139e-9};
const double kGN[] = {-0.000539042911019078575891, -0.28398759004727721098e-6,  0.899465114892291446442e-6,
                      0.229345859265920864296e-7,  0.225561444863500149219e-9,  0.947846627503022684216e-12,
                      0.135880130108924861008e-14, -0.348890393399948882918e-21};
const double kGD[] = {1.0,
                      0.0845746234001899436914,
                      0.00282092984726264681981,
                      0.468292921940894236786e-4,
                      0.399968812193862100054e-6,
                      0.161809290887904476097e-8,
                      0.231558608310259605225e-11};

// statrs erf_inv_impl(p, q, s): p = 1 - q in [0, 1], s the sign.
double erf_inv_impl(double p, double q, double s) {
  double result;
  if (p <= 0.5) {
    const double y = 0.0891314744949340820313;
    const double g = p * (p + 10.0);
    const double r = polynomial(p, kAN) / polynomial(p, kAD);
    result = g * y + g * r;
  } else if (q >= 0.25) {
    const double y = 2.249481201171875;
    const double g = std::sqrt(-2.0 * std::log(q));
    const double xs = q - 0.25;
    const double r = polynomial(xs, kBN) / polynomial(xs, kBD);
    result = g / (y + r);
  } else {
    const double x = std::sqrt(-std::log(q));
    if (x < 3.0) {
      const double y = 0.807220458984375;
      const double xs = x - 1.125;
      const double r = polynomial(xs, kCN) / polynomial(xs, kCD);
      result = y * x + r * x;
    } else if (x < 6.0) {
      const double y = 0.93995571136474609375;
      const double xs = x - 3.0;
      const double r = polynomial(xs, kDN) / polynomial(xs, kDD);
      result = y * x + r * x;
    } else if (x < 18.0) {
      const double y = 0.98362827301025390625;
      const double xs = x - 6.0;
      const double r = polynomial(xs, kEN) / polynomial(xs, kED);
      result = y * x + r * x;
    } else if (x < 44.0) {
      const double y = 0.99714565277099609375;
      const double xs = x - 18.0;
      const double r = polynomial(xs, kFN) / polynomial(xs, kFD);
      result = y * x + r * x;
    } else {
      const double y = 0.99941349029541015625;
      const double xs = x - 44.0;
      const double r = polynomial(xs, kGN) / polynomial(xs, kGD);
      result = y * x + r * x;
    }
  }
  return s * result;
}

// statrs erfc_inv
double erfc_inv(double z) {
  if (z <= 0.0) return std::numeric_limits<double>::infinity();
  if (z >= 2.0) return -std::numeric_limits<double>::infinity();
  if (z > 1.0) {
    const double q = 2.0 - z;
    return erf_inv_impl(1.0 - q, q, -1.0);
  }
  return erf_inv_impl(1.0 - z, z, 1.0);
}

}  // namespace

// statrs Normal::inverse_cdf with mean 0 and std_dev 1: mean - std_dev * SQRT_2 * erfc_inv(2 x)
static double normal_inverse_cdf(double p) {
  if (!(p >= 0.0 && p <= 1.0)) return std::numeric_limits<double>::quiet_NaN();  // statrs panics
  return 0.0 - (1.0 * 1.4142135623730950488016887242097 * erfc_inv(2.0 * p));
}

double remedy_z_score(double confidence_level) {
  double confidence = std::isnan(confidence_level) ? 0.95 : confidence_level;  // analysis.rs:503
  confidence = std::fmin(std::fmax(confidence, 0.50), 0.999);                   // :505
  const double alpha = 1.0 - confidence;
  return normal_inverse_cdf(1.0 - (alpha / 2.0));  // :510-513
}

int remedy_check_shape(int64_t n, int k) {
  if (k < 2) return fail(OB_E_INVALID, "remedy: the design needs the intercept and at least one more column");
  if (k > kRemedyMaxK)
    return fail(OB_E_UNSUPPORTED, "remedy: %d design columns beside the intercept, the kernels take at most %d", k - 1,
                kRemedyMaxK - 1);
  if (n < 0) return fail(OB_E_INVALID, "bad remedy dimensions");
  if (n >= (int64_t)0x7fffffff - 256) return fail(OB_E_UNSUPPORTED, "remedy: too many rows");
  return OB_OK;
}

static const char* const kSingular = "Covariance matrix is singular, likely due to perfect multicollinearity.";

// Design column j (0: the intercept) as a column of the Gram over [features(k - 1), y, 1].
static inline int gram_col(int j, int k) { return j == 0 ? k : j - 1; }

static int remedy_solve(const double* gram_a, const double* gram_fit, int k, double* beta, double* cov) {
  OB_TRY(remedy_check_shape(0, k));
  if (!gram_a || !beta || !cov) return fail(OB_E_INVALID, "null pointer");
  const int k1 = k + 1;
  const double* gf = gram_fit ? gram_fit : gram_a;
  std::vector<double> ma((size_t)k * k), mf((size_t)k * k), inv;
  for (int b = 0; b < k; ++b) {
    for (int a = 0; a < k; ++a) {
      ma[a + (size_t)b * k] = gram_a[gram_col(a, k) + (size_t)gram_col(b, k) * k1];
      mf[a + (size_t)b * k] = gf[gram_col(a, k) + (size_t)gram_col(b, k) * k1];
    }
    beta[b] = gf[gram_col(b, k) + (size_t)(k - 1) * k1];  // X'y: the Gram's y column
  }
  bool finite = true;
  for (double v : ma) finite = finite && std::isfinite(v);
  if (!finite || !try_inverse(ma, k, inv)) return fail(OB_E_LINALG, "%s", kSingular);  // analysis.rs:495-500
  for (double v : inv) finite = finite && std::isfinite(v);
  if (!finite || !chol_factor_solve(mf.data(), k, beta, BackSub::Dot)) return fail(OB_E_LINALG, "%s", kSingular);
  std::copy(inv.begin(), inv.end(), cov);
  return OB_OK;
}

static int remedy_check_request(const ob_remedy_request* rq) {
  if (!rq) return fail(OB_E_INVALID, "null pointer");
  if (rq->strategy != OB_REMEDY_GREEDY && rq->strategy != OB_REMEDY_EQUITABLE) return fail(OB_E_INVALID, "bad strategy");
  if (rq->range_target < OB_REMEDY_MIDPOINT || rq->range_target > OB_REMEDY_UPPER)
    return fail(OB_E_INVALID, "bad range target");
  if (std::isnan(rq->budget) || std::isnan(rq->min_gap_pct)) return fail(OB_E_INVALID, "NaN in the request");
  return OB_OK;
}

static const Col* remedy_column(const Frame& f, const char* name, int* rc) {
  const int ci = name ? f.find(name) : -1;
  if (ci < 0) {
    *rc = fail(OB_E_COLUMN, "Column '%s' not found in dataset.", name ? name : "");  // analysis.rs:336
    return nullptr;
  }
  const Col& c = f.cols[ci];
  for (int64_t r = 0; r < f.nrows; ++r)
    if (!c.valid[r]) {
      *rc = fail(OB_E_INVALID, "null value in column `%s` (row %lld)", c.name.c_str(), (long long)r);
      return nullptr;
    }
  return &c;
}

// The frame checks of ob_remedy_run, shared with ob_remedy_defend: all before any device work, in this order.
// index: the reference group's original rows, then the target group's (analysis.rs:387-398). n_ref: A's rows.
static int remedy_check_frame(const ob_column* cols, int n_cols, int64_t n_rows, const ob_builder_config* cfg, Frame& f,
                              std::vector<int64_t>& index, int64_t* n_ref) {
  if (!cfg || !cfg->outcome || !cfg->group || !cfg->reference_group) return fail(OB_E_INVALID, "null pointer");
  if (cfg->n_predictors < 0 || cfg->n_categorical < 0) return fail(OB_E_INVALID, "bad name list");
  OB_TRY(load_frame(cols, n_cols, n_rows, f));
  int rc = OB_OK;
  const Col* yc = remedy_column(f, cfg->outcome, &rc);
  if (!yc) return rc;
  int64_t width = 1 + cfg->n_predictors;
  for (int p = 0; p < cfg->n_predictors; ++p)
    if (!remedy_column(f, cfg->predictors[p], &rc)) return rc;
  for (int p = 0; p < cfg->n_categorical; ++p) {
    const Col* c = remedy_column(f, cfg->categorical[p], &rc);
    if (!c) return rc;
    if (c->kind == OB_COL_STR) width += (int64_t)std::set<std::string>(c->s.begin(), c->s.end()).size() - 1;
  }
  const Col* gc = remedy_column(f, cfg->group, &rc);
  if (!gc) return rc;
  if (yc->kind == OB_COL_F64)
    for (int64_t r = 0; r < f.nrows; ++r)
      if (!std::isfinite(yc->f[r])) return fail(OB_E_INVALID, "non-finite value in column `%s` (row %lld)", yc->name.c_str(), (long long)r);
  if (gc->kind != OB_COL_STR)  // analysis.rs:379-383: `.str()` of a numeric column fails
    return fail(OB_E_POLARS, "%sinvalid series dtype: expected `String`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                dtype_name(gc->kind), gc->name.c_str());
  const std::set<std::string> levels(gc->s.begin(), gc->s.end());
  if (levels.size() != 2 || !levels.count(cfg->reference_group))
    return fail(OB_E_UNSUPPORTED, "optimize needs exactly two groups, the reference group among them; `%s` has %zu",
                gc->name.c_str(), levels.size());
  if (width > kRemedyMaxK)
    return fail(OB_E_UNSUPPORTED, "remedy: %lld design columns beside the intercept, the kernels take at most %d",
                (long long)(width - 1), kRemedyMaxK - 1);
  index.clear();
  index.reserve((size_t)f.nrows);
  for (int pass = 0; pass < 2; ++pass)
    for (int64_t r = 0; r < f.nrows; ++r)
      if ((gc->s[r] == cfg->reference_group) == (pass == 0)) index.push_back(r);
  *n_ref = 0;
  for (int64_t r = 0; r < f.nrows; ++r) *n_ref += gc->s[r] == cfg->reference_group;
  return OB_OK;
}

static int remedy_run(ob_ctx* ctx, const ob_column* cols, int n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_remedy_request* rq, int target, int want_contrib, ob_remedy_results** out) {
  if (out) *out = nullptr;
  OB_TRY(remedy_check_request(rq));
  if (target != OB_REMEDY_TARGET_REFERENCE && target != OB_REMEDY_TARGET_POOLED) return fail(OB_E_INVALID, "bad target");
  Frame f;
  std::vector<int64_t> index;
  int64_t n_ref = 0;
  int rc = OB_OK;
  OB_TRY(remedy_check_frame(cols, n_cols, n_rows, cfg, f, index, &n_ref));
  if (!ctx || !out) return fail(OB_E_INVALID, "null pointer");

  ob_builder_config c2 = *cfg;
  c2.reference_coeffs = 2;  // ReferenceCoefficients::Pooled (analysis.rs:354, 372)
  c2.bootstrap_reps = 0;    // the reference's 10 replicates are never read
  ob_matrices* mats = nullptr;
  OB_TRY(ob_builder_data_matrices(cols, n_cols, n_rows, &c2, &mats));
  struct Free {
    ob_matrices* m;
    ~Free() { ob_matrices_free(m); }
  } free_mats{mats};
  // the crate's B is the reference group (builder.rs:61-102): the engine's A (analysis.rs:409)
  int64_t n_b = 0, n_a = 0;
  int32_t k = 0;
  const double *xt = nullptr, *yt = nullptr, *xr = nullptr, *yr = nullptr;
  OB_TRY(ob_matrices_dims(mats, &n_b, &n_a, &k));
  OB_TRY(ob_matrices_get(mats, &xt, &yt, &xr, &yr));
  const int64_t n = n_a + n_b;
  OB_TRY(remedy_check_shape(n, k));
  if (n != (int64_t)index.size()) return fail(OB_E_INVALID, "rows were dropped while cleaning the frame");
  if (n_ref != n_a) return fail(OB_E_INVALID, "rows were dropped while cleaning the frame");
  ob_results* point = nullptr;
  OB_TRY(ob_builder_run(ctx, cols, n_cols, n_rows, &c2, &point));
  const double original_gap = ob_results_total_gap(point);  // analysis.rs:361-362
  ob_results_free(point);

  // one upload: [features, y] column-major, A's rows first
  std::vector<double> xy((size_t)n * k);
  for (int c = 0; c < k; ++c) {
    double* dst = xy.data() + (size_t)c * n;
    const double* sa = c < k - 1 ? xr + (size_t)(c + 1) * n_a : yr;
    const double* sb = c < k - 1 ? xt + (size_t)(c + 1) * n_b : yt;
    std::copy(sa, sa + n_a, dst);
    std::copy(sb, sb + n_b, dst + n_a);
  }
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dxy, dfair, dlev, dcontrib;
  OB_HIP(dxy.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(dfair.alloc(sizeof(double) * (size_t)n));
  OB_HIP(dlev.alloc(sizeof(double) * (size_t)n));
  if (want_contrib) OB_HIP(dcontrib.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(hipMemcpyAsync(dxy.p, xy.data(), sizeof(double) * (size_t)n * k, hipMemcpyHostToDevice, st));
  const int k1 = k + 1;
  std::vector<double> ga((size_t)k1 * k1), gf, beta(k), cov((size_t)k * k);
  double gram_ms = 0.0, ms = 0.0, score_ms = 0.0, rss = 0.0;
  OB_TRY(vif_gram_device(ctx, dxy.d(), n, n_a, k, ga.data(), &gram_ms));
  if (target == OB_REMEDY_TARGET_POOLED) {  // A's and B's Grams apart, added here: cov needs A's alone
    gf.resize(ga.size());
    OB_TRY(vif_gram_device(ctx, dxy.d() + n_a, n, n_b, k, gf.data(), &ms));
    gram_ms += ms;
    for (size_t i = 0; i < gf.size(); ++i) gf[i] += ga[i];
  }
  OB_TRY(remedy_solve(ga.data(), gf.empty() ? nullptr : gf.data(), k, beta.data(), cov.data()));
  const double* dy = dxy.d() + (size_t)(k - 1) * n;
  OB_TRY(remedy_score_device(ctx, dxy.d(), n, dy, n, n_a, k, beta.data(), cov.data(), dfair.d(), dlev.d(), &rss,
                             want_contrib ? dcontrib.d() : nullptr, &score_ms));
  const double dof = (double)n_a - (double)k;  // analysis.rs:482-489
  const double sigma2 = dof > 0.0 ? rss / dof : 0.0;
  ob_remedy_results* r = new ob_remedy_results();
  rc = remedy_allocate_device(ctx, dy, dfair.d(), dlev.d(), n_a, n_b, index.data(), sigma2, *rq, *r);
  if (rc == OB_OK && want_contrib && !r->row.empty()) {
    std::vector<double> con((size_t)n * k);
    const hipError_t e = hipMemcpy(con.data(), dcontrib.p, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(OB_E_HIP, "HIP error %s", hipGetErrorString(e));
    r->contrib.resize(r->row.size() * (size_t)k);
    for (size_t i = 0; i < r->row.size() && rc == OB_OK; ++i)
      for (int c = 0; c < k; ++c) r->contrib[i * k + c] = con[(size_t)c * n + r->row[i]];
  }
  if (rc != OB_OK) {
    delete r;
    return rc;
  }
  for (int c = 0; c < k; ++c) r->names.push_back(ob_matrices_name(mats, c));
  for (const std::string& s : r->names) r->name_ptrs.push_back(s.c_str());
  r->beta = beta;
  r->info.original_gap = original_gap;
  r->info.new_gap = n_b > 0 ? original_gap + r->info.total_cost / (double)n_b : original_gap;  // analysis.rs:841-845
  r->info.gram_ms = gram_ms;
  r->info.score_ms = score_ms;
  *out = r;
  return OB_OK;
}

static int remedy_frontier(ob_ctx* ctx, const ob_column* cols, int n_cols, int64_t n_rows, const ob_builder_config* cfg,
                           int steps, double max_budget, double* budget, double* tstat, double* pval, int32_t* sig,
                           double* ms_out) {
  if (ms_out) ms_out[0] = ms_out[1] = 0.0;
  if (steps < 1) return fail(OB_E_INVALID, "frontier: at least one step");
  if (steps > OB_REMEDY_MAX_STEPS) return fail(OB_E_UNSUPPORTED, "frontier: %d steps, the kernels take at most %d", steps, OB_REMEDY_MAX_STEPS);
  if (!budget || !tstat || !pval || !sig) return fail(OB_E_INVALID, "null pointer");
  // analysis.rs:928-946: budget 0, Reference, Greedy, Midpoint, every other switch at its default
  ob_remedy_request rq = {};
  rq.confidence_level = 0.95;
  ob_remedy_results* opt = nullptr;
  OB_TRY(remedy_run(ctx, cols, n_cols, n_rows, cfg, &rq, OB_REMEDY_TARGET_REFERENCE, 0, &opt));
  struct FreeOpt {
    ob_remedy_results* r;
    ~FreeOpt() { delete r; }
  } free_opt{opt};
  const double total_need = opt->info.required_budget;
  double mb = std::isnan(max_budget) ? total_need * 1.1 : max_budget;  // :948
  if (mb < 1e-9) mb = 1000.0;                                           // :1032-1036
  const double step = mb / (double)steps;
  const int s = steps + 1;

  ob_builder_config c2 = *cfg;
  c2.reference_coeffs = 2;
  c2.bootstrap_reps = 0;
  ob_matrices* mats = nullptr;
  OB_TRY(ob_builder_data_matrices(cols, n_cols, n_rows, &c2, &mats));
  struct Free {
    ob_matrices* m;
    ~Free() { ob_matrices_free(m); }
  } free_mats{mats};
  int64_t n_b = 0, n_a = 0;
  int32_t k = 0;
  const double *xt = nullptr, *yt = nullptr, *xr = nullptr, *yr = nullptr;
  OB_TRY(ob_matrices_dims(mats, &n_b, &n_a, &k));
  OB_TRY(ob_matrices_get(mats, &xt, &yt, &xr, &yr));
  const int64_t n = n_a + n_b;
  const int k1 = k + 1;
  // pending payments (:1066-1081): the adjustments in index order, sorted by gap descending, stable; the running
  // prefix in that order, one by one
  const size_t m = opt->row.size();
  std::vector<uint32_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return opt->adjustment[a] > opt->adjustment[b]; });
  std::vector<double> dense(2 * (size_t)n, 0.0);  // gap[n], then pre[n]
  double run = 0.0;
  for (size_t c = 0; c < m; ++c) {
    const int64_t row = opt->row[order[c]];
    dense[row] = opt->adjustment[order[c]];
    dense[(size_t)n + row] = run;
    run += opt->adjustment[order[c]];
  }
  std::vector<double> xy((size_t)n * k);
  for (int c = 0; c < k; ++c) {
    double* dst = xy.data() + (size_t)c * n;
    const double* sa = c < k - 1 ? xr + (size_t)(c + 1) * n_a : yr;
    const double* sb = c < k - 1 ? xt + (size_t)(c + 1) * n_b : yt;
    std::copy(sa, sa + n_a, dst);
    std::copy(sb, sb + n_b, dst + n_a);
  }
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dxy, dd;
  OB_HIP(dxy.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(dd.alloc(sizeof(double) * 2 * (size_t)n));
  OB_HIP(hipMemcpyAsync(dxy.p, xy.data(), sizeof(double) * (size_t)n * k, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemcpyAsync(dd.p, dense.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
  // X_p'X_p from A's and B's Grams over [features, y, 1]: the dummy's row is B's ones row
  const int kg = k + 1;
  std::vector<double> ga((size_t)kg * kg), gb((size_t)kg * kg), xtx((size_t)k1 * k1), inv;
  OB_TRY(vif_gram_device(ctx, dxy.d(), n, n_a, k, ga.data(), nullptr));
  OB_TRY(vif_gram_device(ctx, dxy.d() + n_a, n, n_b, k, gb.data(), nullptr));
  auto gcol = [&](int c) { return c == 0 ? k : c - 2; };  // pooled column (not the dummy) as a Gram column
  for (int a = 0; a < k1; ++a)
    for (int b = 0; b < k1; ++b) {
      double v;
      if (a == 1 || b == 1) {
        const int o = a == 1 ? b : a;
        v = o == 1 ? gb[k + (size_t)k * kg] : gb[gcol(o) + (size_t)k * kg];
      } else {
        v = ga[gcol(a) + (size_t)gcol(b) * kg] + gb[gcol(a) + (size_t)gcol(b) * kg];
      }
      xtx[a + (size_t)b * k1] = v;
    }
  if (!try_inverse(xtx, k1, inv)) return fail(OB_E_LINALG, "Singular matrix in Pooled OLS");  // :1024
  const double* dy = dxy.d() + (size_t)(k - 1) * n;
  std::vector<double> xty((size_t)k1 * s), beta((size_t)k1 * s), rss(s);
  double ms0 = 0.0, ms1 = 0.0;
  OB_TRY(remedy_front_xty_device(ctx, dxy.d(), n, dy, dd.d(), dd.d() + n, n, n_a, k, s, step, xty.data(), &ms0));
  for (int j = 0; j < s; ++j)
    for (int a = 0; a < k1; ++a) {
      double v = 0.0;
      for (int b = 0; b < k1; ++b) v += inv[a + (size_t)b * k1] * xty[(size_t)b * s + j];
      beta[a + (size_t)j * k1] = v;
    }
  OB_TRY(remedy_front_rss_device(ctx, dxy.d(), n, dy, dd.d(), dd.d() + n, n, n_a, k, s, step, beta.data(), rss.data(), &ms1));
  if (ms_out) {
    ms_out[0] = ms0;
    ms_out[1] = ms1;
  }
  const double dof = (double)n - (double)k1;  // :1091
  for (int j = 0; j < s; ++j) {
    budget[j] = j == 0 ? 0.0 : (double)j * step;
    if (dof <= 0.0) {
      tstat[j] = 0.0;
      pval[j] = 1.0;
      sig[j] = 0;
      continue;
    }
    const double sigma_sq = rss[j] / dof;
    const double se_group = std::sqrt(sigma_sq * inv[1 + (size_t)1 * k1]);
    const double t = beta[1 + (size_t)j * k1] / se_group;
    const double p = 2.0 * (0.5 * std::erfc(std::fabs(t) / 1.4142135623730950488016887242097));  // statrs cdf(-|t|)
    tstat[j] = t;
    pval[j] = p;
    sig[j] = p < 0.05;
  }
  return OB_OK;
}

// ---- check_defensibility_inner (engine/src/defensibility.rs) and verify_inner (analysis.rs:40-96) -----------

// The checks of the array pass that need no device, in the order the header gives.
static int defend_check_arrays(const double* y, const double* fair, const double* lev, int64_t n_a, int64_t n_b,
                               const int64_t* rows, const double* values, int64_t m, double sigma2) {
  if (n_a < 0 || n_b < 0 || m < 0) return fail(OB_E_INVALID, "bad remedy dimensions");
  OB_TRY(remedy_check_shape(n_a + n_b, 2));
  if (m >= (int64_t)0x7fffffff) return fail(OB_E_UNSUPPORTED, "defend: too many adjustments");
  const int64_t n = n_a + n_b;
  if ((n > 0 && (!y || !fair || !lev)) || (m > 0 && (!rows || !values))) return fail(OB_E_INVALID, "null pointer");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i]) || !std::isfinite(fair[i]) || !std::isfinite(lev[i]))
      return fail(OB_E_INVALID, "non-finite wage, fair wage or leverage (row %lld)", (long long)i);
  if (std::isnan(sigma2)) return fail(OB_E_INVALID, "NaN sigma_squared");
  for (int64_t j = 0; j < m; ++j) {
    if (rows[j] < 0 || rows[j] >= n)
      return fail(OB_E_INVALID, "adjustment %lld names stacked row %lld outside [0, %lld)", (long long)j, (long long)rows[j], (long long)n);
    if (!std::isfinite(values[j])) return fail(OB_E_INVALID, "non-finite adjustment value (adjustment %lld)", (long long)j);
  }
  return OB_OK;
}

struct OverrideCell {
  int64_t row;
  int pred;
  double value;
};

// defensibility.rs:32-73. The flat list keeps every name, a predictor or not: a set of ignored names still
// replaces the row's earlier set, as the reference's insert does.
static int resolve_overrides(const int64_t* index, int64_t m, const int64_t* opos, const char* const* oname,
                             const double* ovalue, int64_t n_ovr, const char* const* preds, int n_preds, int64_t n_rows,
                             std::vector<OverrideCell>& cells) {
  cells.clear();
  if (m < 0 || n_ovr < 0 || n_preds < 0) return fail(OB_E_INVALID, "bad override list");
  if ((m > 0 && !index) || (n_ovr > 0 && (!opos || !oname || !ovalue)) || (n_preds > 0 && !preds)) return fail(OB_E_INVALID, "null pointer");
  for (int64_t i = 0; i < n_ovr; ++i) {
    if (opos[i] < 0 || opos[i] >= m) return fail(OB_E_INVALID, "override %lld names adjustment %lld of %lld", (long long)i, (long long)opos[i], (long long)m);
    if (!oname[i]) return fail(OB_E_INVALID, "null pointer");
    if (!std::isfinite(ovalue[i])) return fail(OB_E_INVALID, "non-finite override value for `%s` (adjustment %lld)", oname[i], (long long)opos[i]);
  }
  // entries by adjustment position, stable: the sets in request order, a set's names in the order given
  std::vector<int64_t> order((size_t)n_ovr);
  for (int64_t i = 0; i < n_ovr; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return opos[a] < opos[b]; });
  std::map<int64_t, std::map<std::string, double>> by_index;  // HashMap<usize, HashMap<String, f64>>
  for (size_t a = 0; a < order.size();) {
    size_t b = a;
    std::map<std::string, double> set;
    while (b < order.size() && opos[order[b]] == opos[order[a]]) {
      set[oname[order[b]]] = ovalue[order[b]];
      ++b;
    }
    by_index[index[opos[order[a]]]] = std::move(set);  // the last set for an index wins as a whole
    a = b;
  }
  for (int p = 0; p < n_preds; ++p) {
    if (!preds[p]) return fail(OB_E_INVALID, "null pointer");
    for (const auto& kv : by_index) {
      if (kv.first < 0 || kv.first >= n_rows) continue;  // :59
      const auto it = kv.second.find(preds[p]);
      if (it != kv.second.end()) cells.push_back({kv.first, p, it->second});
    }
  }
  return OB_OK;
}

static int apply_adjustments(const double* wage, const uint8_t* valid, int64_t n_rows, const int64_t* index,
                             const double* value, int64_t m, double* out) {
  if (n_rows < 0 || m < 0) return fail(OB_E_INVALID, "bad remedy dimensions");
  if ((n_rows > 0 && (!wage || !out)) || (m > 0 && (!index || !value))) return fail(OB_E_INVALID, "null pointer");
  std::copy(wage, wage + n_rows, out);
  for (int64_t j = 0; j < m; ++j) {
    if (index[j] < 0 || index[j] >= n_rows)  // analysis.rs:81-87
      return fail(OB_E_INVALID, "Adjustment index %lld is out of bounds (dataset has %lld rows)", (long long)index[j], (long long)n_rows);
    if (!std::isfinite(value[j])) return fail(OB_E_INVALID, "non-finite adjustment value (adjustment %lld)", (long long)j);
    if (!valid || valid[index[j]]) out[index[j]] = out[index[j]] + value[j];  // :78-80, one by one
  }
  return OB_OK;
}

static int remedy_defend(ob_ctx* ctx, const ob_column* cols, int n_cols, int64_t n_rows, const ob_builder_config* cfg,
                         const int64_t* index_in, const double* value, int64_t m, const int64_t* opos,
                         const char* const* oname, const double* ovalue, int64_t n_ovr, double confidence_level,
                         int want_contrib, ob_remedy_results** out) {
  if (out) *out = nullptr;
  if (m < 0 || n_ovr < 0) return fail(OB_E_INVALID, "bad adjustment list");
  if ((m > 0 && (!index_in || !value)) || (n_ovr > 0 && (!opos || !oname || !ovalue))) return fail(OB_E_INVALID, "null pointer");
  if (m >= (int64_t)0x7fffffff) return fail(OB_E_UNSUPPORTED, "defend: too many adjustments");
  Frame f;
  std::vector<int64_t> index;
  int64_t n_ref = 0;
  OB_TRY(remedy_check_frame(cols, n_cols, n_rows, cfg, f, index, &n_ref));
  for (int64_t j = 0; j < m; ++j)
    if (!std::isfinite(value[j])) return fail(OB_E_INVALID, "non-finite adjustment value (adjustment %lld)", (long long)j);
  std::vector<OverrideCell> cells;
  OB_TRY(resolve_overrides(index_in, m, opos, oname, ovalue, n_ovr, cfg->predictors, cfg->n_predictors, f.nrows, cells));
  if (!ctx || !out) return fail(OB_E_INVALID, "null pointer");

  // the touched predictor columns, copied as f64 and edited; every other column is the caller's
  std::vector<ob_column> cols2(cols, cols + n_cols);
  std::vector<std::vector<double>> edited;
  edited.reserve(cells.size());
  for (size_t c = 0; c < cells.size();) {
    const int p = cells[c].pred;
    const int ci = f.find(cfg->predictors[p]);
    const Col& src = f.cols[ci];
    size_t e = c;
    while (e < cells.size() && cells[e].pred == p) ++e;
    if (src.kind != OB_COL_STR) {  // `.f64()` of a string column fails and the reference goes on (:53)
      edited.emplace_back((size_t)f.nrows);
      std::vector<double>& v = edited.back();
      for (int64_t r = 0; r < f.nrows; ++r) v[r] = src.kind == OB_COL_F64 ? src.f[r] : (double)src.i[r];
      for (size_t q = c; q < e; ++q) v[cells[q].row] = cells[q].value;
      for (int j = 0; j < n_cols; ++j)  // a predictor named twice edits one column
        if (src.name == cols[j].name) {
          cols2[j].kind = OB_COL_F64;
          cols2[j].f64 = v.data();
          cols2[j].i64 = nullptr;
        }
    }
    c = e;
  }

  ob_builder_config c2 = *cfg;
  c2.reference_coeffs = 2;  // ReferenceCoefficients::Pooled (defensibility.rs:95); the matrices do not depend on it
  c2.bootstrap_reps = 0;
  ob_matrices* mats = nullptr;
  OB_TRY(ob_builder_data_matrices(cols2.data(), n_cols, n_rows, &c2, &mats));
  struct Free {
    ob_matrices* m;
    ~Free() { ob_matrices_free(m); }
  } free_mats{mats};
  int64_t n_b = 0, n_a = 0;
  int32_t k = 0;
  const double *xt = nullptr, *yt = nullptr, *xr = nullptr, *yr = nullptr;
  OB_TRY(ob_matrices_dims(mats, &n_b, &n_a, &k));
  OB_TRY(ob_matrices_get(mats, &xt, &yt, &xr, &yr));
  const int64_t n = n_a + n_b;
  OB_TRY(remedy_check_shape(n, k));
  if (n != (int64_t)index.size() || n_ref != n_a) return fail(OB_E_INVALID, "rows were dropped while cleaning the frame");
  // original index -> stacked row; an index outside the frame is skipped (:200)
  std::vector<int64_t> inverse((size_t)f.nrows, -1), rows, kept_index;
  std::vector<double> kept_value;
  for (int64_t s = 0; s < n; ++s) inverse[index[s]] = s;
  int64_t n_skipped = 0;
  for (int64_t j = 0; j < m; ++j) {
    const int64_t s = index_in[j] >= 0 && index_in[j] < f.nrows ? inverse[index_in[j]] : -1;
    if (s < 0) {
      ++n_skipped;
      continue;
    }
    rows.push_back(s);
    kept_index.push_back(index_in[j]);
    kept_value.push_back(value[j]);
  }

  std::vector<double> xy((size_t)n * k);  // one upload: [features, y] column-major, A's rows first
  for (int c = 0; c < k; ++c) {
    double* dst = xy.data() + (size_t)c * n;
    const double* sa = c < k - 1 ? xr + (size_t)(c + 1) * n_a : yr;
    const double* sb = c < k - 1 ? xt + (size_t)(c + 1) * n_b : yt;
    std::copy(sa, sa + n_a, dst);
    std::copy(sb, sb + n_b, dst + n_a);
  }
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dxy, dfair, dlev, dcontrib;
  OB_HIP(dxy.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(dfair.alloc(sizeof(double) * (size_t)n));
  OB_HIP(dlev.alloc(sizeof(double) * (size_t)n));
  if (want_contrib) OB_HIP(dcontrib.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(hipMemcpyAsync(dxy.p, xy.data(), sizeof(double) * (size_t)n * k, hipMemcpyHostToDevice, st));
  const int k1 = k + 1;
  std::vector<double> ga((size_t)k1 * k1), beta(k), cov((size_t)k * k);
  double gram_ms = 0.0, score_ms = 0.0, rss = 0.0;
  OB_TRY(vif_gram_device(ctx, dxy.d(), n, n_a, k, ga.data(), &gram_ms));
  OB_TRY(remedy_solve(ga.data(), nullptr, k, beta.data(), cov.data()));
  const double* dy = dxy.d() + (size_t)(k - 1) * n;
  OB_TRY(remedy_score_device(ctx, dxy.d(), n, dy, n, n_a, k, beta.data(), cov.data(), dfair.d(), dlev.d(), &rss,
                             want_contrib ? dcontrib.d() : nullptr, &score_ms));
  const double dof = (double)n_a - (double)k;  // defensibility.rs:135-140
  const double sigma2 = dof > 0.0 ? rss / dof : 0.0;
  ob_remedy_results* r = new ob_remedy_results();
  int rc = remedy_defend_device(ctx, dy, dfair.d(), dlev.d(), n_a, n_b, rows.data(), kept_value.data(), (int64_t)rows.size(),
                                sigma2, confidence_level, *r);
  if (rc == OB_OK && want_contrib && !r->row.empty()) {
    std::vector<double> con((size_t)n * k);
    const hipError_t e = hipMemcpy(con.data(), dcontrib.p, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(OB_E_HIP, "HIP error %s", hipGetErrorString(e));
    r->contrib.resize(r->row.size() * (size_t)k);
    for (size_t i = 0; i < r->row.size() && rc == OB_OK; ++i)
      for (int c = 0; c < k; ++c) r->contrib[i * k + c] = con[(size_t)c * n + r->row[i]];
  }
  if (rc != OB_OK) {
    delete r;
    return rc;
  }
  r->index = kept_index;
  for (int c = 0; c < k; ++c) r->names.push_back(ob_matrices_name(mats, c));
  for (const std::string& s : r->names) r->name_ptrs.push_back(s.c_str());
  r->beta = beta;
  r->dinfo.n_skipped = n_skipped;
  r->dinfo.gram_ms = gram_ms;
  r->dinfo.score_ms = score_ms;
  r->info.gram_ms = gram_ms;
  r->info.score_ms = score_ms;
  *out = r;
  return OB_OK;
}

static int remedy_verify(ob_ctx* ctx, const ob_column* cols, int n_cols, int64_t n_rows, const ob_builder_config* cfg,
                         const int64_t* index, const double* value, int64_t m, ob_results** out) {
  if (out) *out = nullptr;
  if (!cfg || !cfg->outcome) return fail(OB_E_INVALID, "null pointer");
  Frame f;
  OB_TRY(load_frame(cols, n_cols, n_rows, f));
  const int ci = f.find(cfg->outcome);
  if (ci < 0) return fail(OB_E_COLUMN, "Column '%s' not found in dataset.", cfg->outcome);  // analysis.rs:64
  const Col& yc = f.cols[ci];
  if (yc.kind == OB_COL_STR) return fail(OB_E_POLARS, "%sColumn '%s' contains non-numeric data.", error_prefix(OB_E_POLARS), cfg->outcome);
  std::vector<double> wage((size_t)f.nrows), adjusted((size_t)f.nrows);
  for (int64_t r = 0; r < f.nrows; ++r) wage[r] = yc.kind == OB_COL_F64 ? yc.f[r] : (double)yc.i[r];
  OB_TRY(apply_adjustments(wage.data(), yc.valid.data(), f.nrows, index, value, m, adjusted.data()));
  if (!ctx || !out) return fail(OB_E_INVALID, "null pointer");
  std::vector<ob_column> cols2(cols, cols + n_cols);
  for (int j = 0; j < n_cols; ++j)
    if (yc.name == cols[j].name) {
      cols2[j].kind = OB_COL_F64;
      cols2[j].f64 = adjusted.data();
      cols2[j].i64 = nullptr;
    }
  return ob_builder_run(ctx, cols2.data(), n_cols, n_rows, cfg, out);
}

}  // namespace ob

extern "C" {

int ob_remedy_frontier(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                       int32_t steps, double max_budget, double* budget, double* t_statistic, double* p_value,
                       int32_t* is_significant, double* ms) {
  return ob::remedy_frontier(ctx, cols, n_cols, n_rows, cfg, steps, max_budget, budget, t_statistic, p_value,
                             is_significant, ms);
}

int ob_remedy_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                  const ob_remedy_request* request, int32_t target, int32_t contributions, ob_remedy_results** out) {
  return ob::remedy_run(ctx, cols, n_cols, n_rows, cfg, request, target, contributions, out);
}

int ob_remedy_results_model(const ob_remedy_results* r, int32_t* k, const char* const** names, const double** beta,
                            const double** contributions) {
  if (!r) return ob::fail(OB_E_INVALID, "null pointer");
  if (k) *k = (int32_t)r->beta.size();
  if (names) *names = r->name_ptrs.data();
  if (beta) *beta = r->beta.data();
  if (contributions) *contributions = r->contrib.empty() ? nullptr : r->contrib.data();
  return OB_OK;
}

double ob_normal_inverse_cdf(double p) { return ob::normal_inverse_cdf(p); }

int ob_remedy_solve(const double* gram_a, const double* gram_fit, int32_t k, double* beta, double* cov) {
  return ob::remedy_solve(gram_a, gram_fit, k, beta, cov);
}

int ob_remedy_score(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int64_t n_rss, int32_t k,
                    const double* beta, const double* cov, double* fair, double* leverage, double* rss,
                    double* contrib) {
  using namespace ob;
  OB_TRY(remedy_check_shape(n, k));
  if (!ctx || !x || !beta || !cov || !fair || !leverage) return fail(OB_E_INVALID, "null pointer");
  if (ldx < n || n_rss < 0 || n_rss > n || (n_rss > 0 && !y)) return fail(OB_E_INVALID, "bad remedy dimensions");
  if (rss) *rss = 0.0;
  if (n == 0) return OB_OK;
  const int p = k - 1;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dx, dy, dfair, dlev, dcontrib;
  OB_HIP(dx.alloc(sizeof(double) * (size_t)n * p));
  OB_HIP(dfair.alloc(sizeof(double) * (size_t)n));
  OB_HIP(dlev.alloc(sizeof(double) * (size_t)n));
  OB_HIP(hipMemcpy2DAsync(dx.p, sizeof(double) * (size_t)n, x, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)n,
                          (size_t)p, hipMemcpyHostToDevice, st));
  if (n_rss > 0) {
    OB_HIP(dy.alloc(sizeof(double) * (size_t)n_rss));
    OB_HIP(hipMemcpyAsync(dy.p, y, sizeof(double) * (size_t)n_rss, hipMemcpyHostToDevice, st));
  }
  if (contrib) OB_HIP(dcontrib.alloc(sizeof(double) * (size_t)n * k));
  OB_TRY(remedy_score_device(ctx, dx.d(), n, n_rss > 0 ? dy.d() : nullptr, n, n_rss, k, beta, cov, dfair.d(), dlev.d(),
                             rss, contrib ? dcontrib.d() : nullptr, nullptr));
  OB_HIP(hipMemcpyAsync(fair, dfair.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  OB_HIP(hipMemcpyAsync(leverage, dlev.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (contrib) OB_HIP(hipMemcpyAsync(contrib, dcontrib.p, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  return OB_OK;
}

int ob_remedy_allocate(ob_ctx* ctx, const double* y, const double* fair, const double* leverage, int64_t n_a,
                       int64_t n_b, const int64_t* index, double sigma_squared, const ob_remedy_request* request,
                       ob_remedy_results** out) {
  using namespace ob;
  if (out) *out = nullptr;
  OB_TRY(remedy_check_request(request));
  if (n_a < 0 || n_b < 0) return fail(OB_E_INVALID, "bad remedy dimensions");
  OB_TRY(remedy_check_shape(n_a + n_b, 2));
  const int64_t n = n_a + n_b;
  if (n > 0 && (!y || !fair || !leverage)) return fail(OB_E_INVALID, "null pointer");
  if (index)
    for (int64_t i = 0; i < n; ++i)
      if (index[i] < 0) return fail(OB_E_INVALID, "negative original index (row %lld)", (long long)i);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i]) || !std::isfinite(fair[i]) || !std::isfinite(leverage[i]))
      return fail(OB_E_INVALID, "non-finite wage, fair wage or leverage (row %lld)", (long long)i);
  if (std::isnan(sigma_squared)) return fail(OB_E_INVALID, "NaN sigma_squared");
  if (!ctx || !out) return fail(OB_E_INVALID, "null pointer");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d;  // y, fair and leverage side by side
  OB_HIP(d.alloc(sizeof(double) * 3 * (size_t)n));
  const double* src[3] = {y, fair, leverage};
  for (int i = 0; i < 3 && n > 0; ++i)
    OB_HIP(hipMemcpyAsync(d.d() + (size_t)i * n, src[i], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  ob_remedy_results* r = new ob_remedy_results();
  const int rc = remedy_allocate_device(ctx, d.d(), d.d() + n, d.d() + 2 * (size_t)n, n_a, n_b, index, sigma_squared,
                                        *request, *r);
  (void)hipStreamSynchronize(st);
  if (rc != OB_OK) {
    delete r;
    return rc;
  }
  *out = r;
  return OB_OK;
}

int ob_remedy_results_info(const ob_remedy_results* r, ob_remedy_info* out) {
  if (!r || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = r->info;
  return OB_OK;
}

int ob_remedy_results_get(const ob_remedy_results* r, const int64_t** index, const double** adjustment,
                          const double** current_wage, const double** new_wage, const double** fair_wage,
                          const double** lower, const double** upper, const int32_t** group, const int64_t** row) {
  if (!r) return ob::fail(OB_E_INVALID, "null pointer");
  if (index) *index = r->index.data();
  if (adjustment) *adjustment = r->adjustment.data();
  if (current_wage) *current_wage = r->current_wage.data();
  if (new_wage) *new_wage = r->new_wage.data();
  if (fair_wage) *fair_wage = r->fair_wage.data();
  if (lower) *lower = r->lower.data();
  if (upper) *upper = r->upper.data();
  if (group) *group = r->group.data();
  if (row) *row = r->row.data();
  return OB_OK;
}

void ob_remedy_results_free(ob_remedy_results* r) { delete r; }

int ob_remedy_defend_rows(ob_ctx* ctx, const double* y, const double* fair, const double* leverage, int64_t n_a,
                          int64_t n_b, const int64_t* rows, const double* values, int64_t m, double sigma_squared,
                          double confidence_level, ob_remedy_results** out) {
  using namespace ob;
  if (out) *out = nullptr;
  OB_TRY(defend_check_arrays(y, fair, leverage, n_a, n_b, rows, values, m, sigma_squared));
  if (!ctx || !out) return fail(OB_E_INVALID, "null pointer");
  const int64_t n = n_a + n_b;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d;  // y, fair and leverage side by side
  OB_HIP(d.alloc(sizeof(double) * 3 * (size_t)n));
  const double* src[3] = {y, fair, leverage};
  for (int i = 0; i < 3 && n > 0; ++i)
    OB_HIP(hipMemcpyAsync(d.d() + (size_t)i * n, src[i], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  ob_remedy_results* r = new ob_remedy_results();
  const int rc = remedy_defend_device(ctx, d.d(), d.d() + n, d.d() + 2 * (size_t)n, n_a, n_b, rows, values, m, sigma_squared,
                                      confidence_level, *r);
  (void)hipStreamSynchronize(st);
  if (rc != OB_OK) {
    delete r;
    return rc;
  }
  *out = r;
  return OB_OK;
}

int ob_remedy_defend(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                     const int64_t* index, const double* value, int64_t m, const int64_t* override_adjustment,
                     const char* const* override_name, const double* override_value, int64_t n_overrides,
                     double confidence_level, int32_t contributions, ob_remedy_results** out) {
  return ob::remedy_defend(ctx, cols, n_cols, n_rows, cfg, index, value, m, override_adjustment, override_name,
                           override_value, n_overrides, confidence_level, contributions, out);
}

int ob_remedy_resolve_overrides(const int64_t* index, int64_t m, const int64_t* override_adjustment,
                                const char* const* override_name, const double* override_value, int64_t n_overrides,
                                const char* const* predictors, int32_t n_predictors, int64_t n_rows, int64_t* out_row,
                                int32_t* out_predictor, double* out_value, int64_t* n_out) {
  using namespace ob;
  if (!n_out || (n_overrides > 0 && (!out_row || !out_predictor || !out_value))) return fail(OB_E_INVALID, "null pointer");
  *n_out = 0;
  std::vector<OverrideCell> cells;
  OB_TRY(resolve_overrides(index, m, override_adjustment, override_name, override_value, n_overrides, predictors,
                           n_predictors, n_rows, cells));
  for (size_t i = 0; i < cells.size(); ++i) {
    out_row[i] = cells[i].row;
    out_predictor[i] = cells[i].pred;
    out_value[i] = cells[i].value;
  }
  *n_out = (int64_t)cells.size();
  return OB_OK;
}

int ob_remedy_results_defensible(const ob_remedy_results* r, const int32_t** is_defensible) {
  if (!r || !is_defensible) return ob::fail(OB_E_INVALID, "null pointer");
  *is_defensible = r->defend ? r->defensible.data() : nullptr;
  return OB_OK;
}

int ob_remedy_results_defend_info(const ob_remedy_results* r, ob_defend_info* out) {
  if (!r || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (!r->defend) return ob::fail(OB_E_INVALID, "not a defensibility handle");
  *out = r->dinfo;
  return OB_OK;
}

int ob_remedy_apply_adjustments(const double* wage, const uint8_t* valid, int64_t n_rows, const int64_t* index,
                                const double* value, int64_t m, double* out) {
  return ob::apply_adjustments(wage, valid, n_rows, index, value, m, out);
}

int ob_remedy_verify(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                     const int64_t* index, const double* value, int64_t m, ob_results** out) {
  return ob::remedy_verify(ctx, cols, n_cols, n_rows, cfg, index, value, m, out);
}

}  // extern "C"
