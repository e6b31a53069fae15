// ob_nopo.hpp -- Nopo's exact-matching decomposition with a bootstrapped common support (Nopo 2008, Stata's
// `nopomatch`): limits, row layout, and the host side that ob_builder.cpp holds (the cells, the
// fragment tables, the aggregation). ob_nopo.hip holds the device side; ob_builder.cpp routes a handle through the
// hooks of ob_model.hpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ob_common.hpp"

struct ob_results;

namespace ob {

struct Config;

// Row (include/oaxaca_boot.h): D, D_X, D_0, D_A, D_B | ybar_A, ybar_B, E_A[y|S], E_B[y|S], CF | the matched shares of
// A and B | the number of support cells.
constexpr int kNopoRowLen = 13;
// The chunk table (ob_engine.hip's make_plan) gives a group min(tiles, max(about 32 tiles_g / tiles, tiles_g / 4096))
// chunks: at most 2048 for a group below 2^31 rows (2^23 tiles), 4096 for both.
constexpr int64_t kNopoMaxChunks = 4096;
// OB_NOPO_MAX_CELLS: a 64-replicate block's table holds N and S per fragment and replicate, 2 x 8 x 64 = 1024 bytes a
// fragment, so the 1 GiB of boot_batch_reps takes 2^20 fragments. A group's rows are sorted by cell, so a cell is one
// run of rows, which the group's chunk boundaries cut into at most one more fragment each: at most n_cells + chunks_g
// - 1 fragments a group, 2 n_cells + 4096 - 2 for both at the worst. (2^20 - 4096) / 2 = 522240 cells always fit.
constexpr int64_t kNopoMaxCells = ((int64_t(1) << 20) - kNopoMaxChunks) / 2;
static_assert(kNopoMaxCells == OB_NOPO_MAX_CELLS, "include/oaxaca_boot.h states the derived limit");

// The checks every entry point makes before any device work.
int nopo_check_shape(int64_t n_cells, int64_t n_a, int64_t n_b);

// One group's rows in stable ascending order of cell id. OBRS-3 position i of the group is its i-th row in that order
// (as the refits' position is the i-th row in order of y): the same seed draws other rows than run() does.
struct NopoGroup {
  std::vector<int64_t> row;   // sorted position -> row of the input frame
  std::vector<int32_t> cell;  // sorted position -> cell id (ascending)
  std::vector<double> y, w;   // sorted; w is empty without a weights column
};
// What nopo_stage makes of a frame and a configuration.
struct NopoStaged {
  int32_t n_cells = 0;
  std::vector<int32_t> row_cell;  // per input row; -1 for a row of neither group
  NopoGroup g[2];                 // A, then B (the reference group)
};
// A group's fragments: the intersections of one cell with one chunk, in row order.
struct NopoFrags {
  std::vector<uint32_t> end;         // [n_frag + 1] the fragment's last row + 1; the last entry is a sentinel
  std::vector<uint32_t> cell;        // [n_frag]
  std::vector<uint32_t> chunk_first; // [chunks of the group] the chunk's first fragment
  std::vector<uint32_t> cell_first;  // [n_cells + 1] the cell's first fragment (a cell without rows: an empty range)
  size_t n() const { return cell.size(); }
};

// Every check of the frame entry points and the cells (include/oaxaca_boot.h), host only. cells_only: stop after the
// refusals and the cell ids (ob_nopo_cells wants the ids alone, also for a frame one of whose groups is empty).
int nopo_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, Config& c,
               NopoStaged& out, bool cells_only);
// chunks: (g, t0, t1) triples of the panel's chunk table, n_chunks of them; the group's are taken.
void nopo_fragments(const std::vector<int32_t>& cell_sorted, int32_t n_cells, const uint32_t* chunks, int n_chunks,
                    uint32_t group, NopoFrags& out);
// finish() on rows of kNopoRowLen doubles and their point row.
int nopo_finish_rows(const double* point, const double* rows, const uint8_t* ok, uint64_t n_reps, ob_results** out);

}  // namespace ob
