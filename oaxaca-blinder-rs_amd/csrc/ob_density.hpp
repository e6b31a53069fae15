// ob_density.hpp -- the bootstrapped DFL density decomposition (DiNardo, Fortin and Lemieux 1996):
// limits and row layout. ob_density.hip holds the device side and the frame entry points; the aggregation of rows
// (density_finish_rows) is host code in ob_builder.cpp, which routes a handle through the hooks of ob_model.hpp.
#pragma once
#include <cstdint>

struct ob_results;

namespace ob {

constexpr int kDensityMaxGrid = 256;  // grid points (OB_DENSITY_MAX_GRID): 16 column tiles, four per wave
// Row (include/oaxaca_boot.h): f_A | f_B | f_C | total | composition | structure (G each) | gamma (K) | effective
// sample size | logit passes.
inline int density_row_len(int k, int G) { return 6 * G + k + 2; }
// The checks every entry point makes before any device work. k: design columns with the intercept.
int density_check_shape(int k, int64_t n_a, int64_t n_b, int G);
// finish() for rows of this layout: the six curves' entries through aggregate(), then the uniform bands.
int density_finish_rows(const double* point, int k, int G, const double* rows, const uint8_t* ok, uint64_t n_reps,
                        ob_results** out);

}  // namespace ob
