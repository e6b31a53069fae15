// ob_frame.hpp -- the column frame the host front ends work on (the stand-in for the polars
// DataFrame). Defined in ob_builder.cpp; ob_dfl.cpp reads frames through the same loader.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ob_common.hpp"

namespace ob {

struct Col {
  std::string name;
  int kind = OB_COL_F64;
  std::vector<double> f;       // OB_COL_F64 values (OB_COL_I64 values cast on use)
  std::vector<int64_t> i;      // OB_COL_I64
  std::vector<std::string> s;  // OB_COL_STR
  std::vector<uint8_t> valid;  // 1 = non-null
};

struct Frame {
  int64_t nrows = 0;
  std::vector<Col> cols;
  int find(const std::string& n) const {
    for (size_t c = 0; c < cols.size(); ++c)
      if (cols[c].name == n) return (int)c;
    return -1;
  }
};

const char* dtype_name(int kind);
// Copies an ob_column array into a Frame (OB_E_INVALID on malformed input, OB_E_POLARS on a
// duplicate column name).
int load_frame(const ob_column* cols, int n_cols, int64_t n_rows, Frame& out);

}  // namespace ob
