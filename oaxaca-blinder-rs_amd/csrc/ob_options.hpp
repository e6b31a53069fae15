// ob_options.hpp -- process-wide engine options for tests and A/B tooling.
//
// The shipped library reads no environment variable: every switch below is set through the C ABI
// (ob_set_option, include/oaxaca_boot.h) by a caller that asks for it -- the parity tests (the f64
// Gram against the i8 Gram, the unreduced Machado-Mata solve against the reduced one, the library
// erfc against npdf_ncdf). A build with -DOB_TUNING=1 (`make tuning`, liboaxaca_boot_tuning.so)
// also reads OB_<NAME> from the environment for an option nobody set, and compiles the timing
// ablation kernels (gram_diag, l1_diag) that the A/B scripts under tools/ drive.
#pragma once

#include <cmath>

#ifndef OB_TUNING
#define OB_TUNING 0
#endif

namespace ob {

enum class Opt : int {
  GramPath,     // 1: f64 MFMA Gram, 2: i8 Gram (an error if its images do not fit); unset: i8 when it fits
  GramDigits,   // 7: seven digit slices on every column tile
  HkErfc,       // 0: the library erfc beside a second exp in the probit/IMR kernels
  MmReduce,     // 0: no Machado-Mata row reduction, 1: always; unset: when both groups have >= 2^16 rows
  MmTrace,      // nonzero: per-iteration Machado-Mata trace on stderr
  MmStateGb,    // Machado-Mata IPM state budget (GB of HBM)
  MmDelta1,     // Machado-Mata start offsets and band parameters (tuning: results do not depend on them)
  MmDelta2,
  MmTol1,
  MmFitStride,
  MmKappa,
  MmBand0,
  GramDiag,     // timing ablations (OB_TUNING builds only): wrong results by design
  L1Diag,
  GramTile,     // i8 Gram kernel: 1 = 8 waves, 32 pairs per block; 2 = 4 waves, 64 pairs (oz_gram_w_kernel);
                // 3 = that wide tile with each chunk's sub-tiles split over two blocks
  DebugCountOverflow,  // nonzero: engine_counts raises its overflow word after the count kernel (tests the
                       // error path that a real count above 255 would take, p < 1e-500 per row)
  RsDouble,     // 1: two count-image / m1 buffers, so a boot's resample runs under the previous Gram;
                // 0: one; unset: the engine's rule (engine_boot)
  MatchChunks,  // the matching distance pass splits the controls into this many chunks (1: no split);
                // unset: the rule of match_knn, a function of the input sizes (results do not depend on it)
  AkmPoll,      // the AKM loops read their done flags every this many iterations (results and iteration
                // counts do not depend on it); unset: kAkmPollDefault
  HkBatch,      // the wide Heckman path (more than 7 selection predictors) runs a segment in batches of this
                // many 64-replicate blocks (rows do not depend on it); unset: the rule of heck_batch
  Count
};

// The option's value, or NaN when it is unset (the caller then uses its built-in default).
double opt(Opt o);

// Convenience: the option as an int / a double, or the default when unset.
inline int opt_int(Opt o, int dflt) {
  const double v = opt(o);
  return std::isnan(v) ? dflt : (int)v;
}
inline double opt_double(Opt o, double dflt) {
  const double v = opt(o);
  return std::isnan(v) ? dflt : v;
}

}  // namespace ob
