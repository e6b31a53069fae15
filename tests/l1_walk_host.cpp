// l1_walk_host.cpp -- host check of ob_spec.h's register-resident Knuth-Yao walk (ob_ky_walk) and
// low popcount (ob_l1_head_bits) against the bit-at-a-time ob_bitstream (tests/test_l1_walk_host.py
// builds and runs it; a stand-alone program, so it may also be built with -fsanitize=...).
//
// Per table t (B(2^(t + 7), 1/2)) it walks every stream twice, once with the generic walk below (the
// stream read through ob_bs_take_msb / ob_bs_bit, the table's full column list) and once with
// ob_ky_walk, and stops at the first differing sample or final bit position:
//   uniform   kUniform streams over varied (q, rep, node, tag, key);
//   found     streams whose walk leaves the hot columns or the stream's first word, searched over
//             (q, rep) with the generic walk until kWant per table or kBudget candidates;
//   crafted   first calls chosen bit by bit so that the walk stays in the tree as long as it can
//             (past the first word, the first call and into a refill), the generic walk reading the
//             same words.
// Prints one line per table and one for the popcounts; exit status 1 on a mismatch, 2 when fewer
// than kFloorTables tables reach kWant found streams.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ob_spec.h"

namespace {

constexpr uint32_t kUniform = 200000, kWant = 16, kFloorTables = 4;
constexpr uint64_t kBudget = 50000000ull;

struct Table {
  uint32_t n = 0, i0 = 0;
  std::vector<uint32_t> off;   // [n + 2] column offsets into list
  std::vector<uint16_t> list;  // column i = 1 .. n: the k with bit n - i of C(n, k) set, ascending
  std::vector<uint32_t> hoff;  // [OB_KY_HOT + 1] hot columns' offsets into hlist
  std::vector<uint16_t> hlist;
};

// the tables as the engine's ky_host builds them: C(n, k) exactly, C(n, k + 1) = C(n, k) (n - k) / (k + 1)
Table build_table(int j) {
  Table t;
  const uint32_t n = 1u << j, L = n / 64 + 1;
  t.n = n;
  std::vector<uint64_t> w((size_t)(n + 1) * L, 0);
  w[0] = 1;
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t* a = &w[(size_t)k * L];
    uint64_t* b = &w[(size_t)(k + 1) * L];
    unsigned __int128 carry = 0;
    for (uint32_t i = 0; i < L; ++i) {
      const unsigned __int128 v = (unsigned __int128)a[i] * (n - k) + carry;
      b[i] = (uint64_t)v;
      carry = v >> 64;
    }
    unsigned __int128 rem = 0;
    for (uint32_t i = L; i-- > 0;) {
      const unsigned __int128 v = (rem << 64) | b[i];
      b[i] = (uint64_t)(v / (k + 1));
      rem = v % (k + 1);
    }
  }
  t.off.assign(n + 2, 0);
  for (uint32_t i = 1; i <= n; ++i) {
    t.off[i] = (uint32_t)t.list.size();
    const uint32_t bit = n - i;
    for (uint32_t k = 0; k <= n; ++k)
      if ((w[(size_t)k * L + bit / 64] >> (bit % 64)) & 1u) t.list.push_back((uint16_t)k);
    if (!t.i0 && t.list.size() > t.off[i]) t.i0 = i;
  }
  t.off[n + 1] = (uint32_t)t.list.size();
  for (uint32_t c = 0; c <= OB_KY_HOT; ++c) t.hoff.push_back(t.off[t.i0 + c] - t.off[t.i0]);
  t.hlist.assign(t.list.begin() + t.off[t.i0], t.list.begin() + t.off[t.i0 + OB_KY_HOT]);
  return t;
}

struct Id {
  uint32_t ctr0, rep, c2, tag, k0, k1;
};

// The generic walk: every bit through the ob_bitstream. `first`, when given, stands for the
// stream's first call (crafted streams); later calls are the stream's own.
uint32_t walk_generic(const Table& t, const Id& id, const ob_u32x4* first, uint32_t* bits) {
  ob_bitstream s = {id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1, 0u, 0u, 0u, 0u, 0u};
  uint32_t d = 0;
  if (first) {
    s.w0 = first->x, s.w1 = first->y, s.w2 = first->z, s.w3 = first->w;
    for (uint32_t b = 0; b + 1 < t.i0; ++b) d = 2u * d + ((first->x >> b) & 1u);
    s.pos = t.i0 - 1u;
  } else {
    d = ob_bs_take_msb(s, t.i0 - 1u);
  }
  for (uint32_t i = t.i0;; ++i) {
    d = 2u * d + ob_bs_bit(s);
    const uint32_t lo = t.off[i], cnt = t.off[i + 1] - lo;
    if (d < cnt) {
      *bits = s.pos;
      return t.list[lo + d];
    }
    d -= cnt;
  }
}

uint32_t walk_fast(const Table& t, const Id& id, const ob_u32x4* first, uint32_t* bits) {
  const ob_u32x4 u = first ? *first : OB_L1_PHILOX(id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1);
  return ob_ky_walk(u, id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1, t.i0, t.hoff.data(), t.hlist.data(),
                    t.off.data(), t.list.data(), bits);
}

bool same(const Table& t, int x, const Id& id, const ob_u32x4* first, const char* kind, uint32_t* bits_out) {
  uint32_t bg = 0, bf = 0;
  const uint32_t g = walk_generic(t, id, first, &bg), f = walk_fast(t, id, first, &bf);
  if (bits_out) *bits_out = bg;
  if (g == f && bg == bf) return true;
  std::printf("MISMATCH table %d %s stream {%u, %u, %u, 0x%x, key %u %u}: generic %u after %u bits, fast %u after %u\n",
              x, kind, id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1, g, bg, f, bf);
  return false;
}

// a first call whose bits keep the walk inside the tree for as long as a bit choice allows, up to 128 bits
ob_u32x4 craft(const Table& t) {
  uint32_t wd[4] = {0, 0, 0, 0};
  uint32_t d = 0;  // the rightmost internal node of every column, as long as there is one
  for (uint32_t b = 0; b < 128u && b + 1u <= t.n; ++b) {
    const uint32_t i = b + 1u, cnt = t.off[i + 1] - t.off[i];
    const uint32_t bit = 2u * d + 1u >= cnt ? 1u : 0u;
    wd[b >> 5] |= bit << (b & 31u);
    d = 2u * d + bit;
    if (d < cnt) break;  // no choice stays in the tree: the walk ends here
    d -= cnt;
  }
  const ob_u32x4 u = {wd[0], wd[1], wd[2], wd[3]};
  return u;
}

}  // namespace

int main() {
  const uint32_t reps[4] = {0u, 9999u, 0x80000011u, 0xFFFFFFFFu};
  int reached = 0;
  for (int x = 0; x < OB_KY_TABLES; ++x) {
    const Table t = build_table(x + OB_KY_MIN_LOG);
    if (!ob_ky_fast_ok(t.i0)) {
      std::printf("table %d: i0 = %u does not fit the first word\n", x, t.i0);
      return 1;
    }
    uint32_t cold = 0, word = 0;
    for (uint32_t s = 0; s < kUniform; ++s) {
      const Id id = {(s % 977u) << 12, reps[s & 3u] + s / 977u, ((s * 2654435761u) >> 7) | (s & 1u),
                     OB_TAG_L1K + ((s >> 2) % 3u << 5) + (s % 19u), 0x0B5EEDu + (s & 4u), (s >> 3) & 1u};
      uint32_t bits;
      if (!same(t, x, id, nullptr, "uniform", &bits)) return 1;
      cold += bits > t.i0 - 1u + OB_KY_HOT;
      word += bits > 32u;
    }
    uint32_t found = 0, found_word = 0;
    uint64_t tried = 0;
    for (; found < kWant && tried < kBudget; ++tried) {
      const Id id = {(uint32_t)(tried & 0xFFFFFu) << 12, 77u + (uint32_t)(tried >> 20), (uint32_t)(2 * x + 1),
                     OB_TAG_L1K + 33u, 0x0B5EEDu, 0u};
      uint32_t bg;
      (void)walk_generic(t, id, nullptr, &bg);
      if (bg <= t.i0 - 1u + OB_KY_HOT) continue;
      if (!same(t, x, id, nullptr, "found", nullptr)) return 1;
      ++found;
      found_word += bg > 32u;
    }
    const ob_u32x4 first = craft(t);
    const Id cid = {5u << 12, 3u, (uint32_t)x, OB_TAG_L1K + 2u, 0x0B5EEDu, 1u};
    uint32_t cbits;
    if (!same(t, x, cid, &first, "crafted", &cbits)) return 1;
    std::printf("table %d (n = %u, i0 = %u): uniform %u (past the hot columns %u, past the first word %u); "
                "found %u past the hot columns in %llu candidates (%u past the first word); crafted walk %u bits\n",
                x, t.n, t.i0, kUniform, cold, word, found, (unsigned long long)tried, found_word, cbits);
    reached += found >= kWant;
  }
  // the low popcount: the first m bits of the stream's first call, m = 1 .. 127
  uint32_t pc = 0;
  for (uint32_t m = 1; m < 128u; ++m)
    for (uint32_t s = 0; s < 2000u; ++s, ++pc) {
      const Id id = {(s % 61u) << 12, reps[s & 3u] + s, (s * 40503u) | 1u, OB_TAG_L1K + (s % 40u), 0x0B5EEDu, s & 1u};
      ob_bitstream bs = {id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1, 0u, 0u, 0u, 0u, 0u};
      const uint32_t g = ob_bs_popcount(bs, m);
      const uint32_t f = ob_l1_head_bits(OB_L1_PHILOX(id.ctr0, id.rep, id.c2, id.tag, id.k0, id.k1), m);
      if (g != f || bs.pos != m) {
        std::printf("MISMATCH popcount m %u stream {%u, %u, %u, 0x%x}: generic %u, fast %u\n", m, id.ctr0, id.rep, id.c2,
                    id.tag, g, f);
        return 1;
      }
    }
  std::printf("popcount: m = 1 .. 127, %u streams, all equal\n", pc);
  std::printf("tables with %u found streams: %d of %d\n", kWant, reached, OB_KY_TABLES);
  return reached >= (int)kFloorTables ? 0 : 2;
}
