// Stand-alone driver of the host side of COO input (fortran_davidson_amd/csrc/coo_host.h): the scalar checks, the search for the
// first offending triple and the stable counting sort by row, on the edge inputs of tests/test_coo_gpu.py - rows of 63, 64, 65, 2048,
// 2049 and 4097 entries in a random order with two empty rows, n = 1 with no triple and with three duplicates, every triple in the
// last row, both index bases, and the refusals (rows -1, n and 0 in base 1, a column out of range, an entry above the diagonal, two
// offenders, nnz = -1, a null array).  The row form is compared with std::stable_sort.  Build and run by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I fortran_davidson_amd/csrc
//       tests/host_sanitizer/coo_driver.cpp -o coo_driver && ./coo_driver
// Exit status 0 and "coo_driver: ok" = every check passed and the sanitizers saw nothing.
#include "coo_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Triples { std::vector<int32_t> row, col; std::vector<double> val; };

static void check_row_form(int64_t n, const Triples& t, int base) {
  const int64_t nnz = (int64_t)t.val.size();
  CooRowForm f;
  coo_row_form(n, nnz, t.row.data(), t.col.data(), t.val.data(), base, f);
  std::vector<int64_t> order((size_t)nnz);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return t.row[(size_t)a] < t.row[(size_t)b]; });
  CHECK((int64_t)f.row_ptr.size() == n + 1 && f.row_ptr[0] == base && f.row_ptr[(size_t)n] == nnz + base);
  CHECK(f.perm == order);
  for (int64_t q = 0; q < nnz; ++q) {
    const size_t p = (size_t)order[(size_t)q];
    CHECK(f.col[(size_t)q] == t.col[p] && f.val[(size_t)q] == t.val[p]);
    const int64_t i = t.row[p] - base;
    CHECK(f.row_ptr[(size_t)i] - base <= q && q < f.row_ptr[(size_t)i + 1] - base);
  }
}

int main() {
  std::mt19937_64 rng(3);
  // rows at the edges of the sorts
  {
    const int64_t n = 4200;
    Triples t;
    for (int64_t i = 0; i < n; ++i) {
      if (i == 100 || i == 101) continue;
      const bool special = i == 63 || i == 64 || i == 65 || i == 2048 || i == 2049 || i == 4097;
      if (!special) { t.row.push_back((int32_t)i); t.col.push_back((int32_t)i); t.val.push_back(10.0 + (double)i); continue; }
      std::vector<int32_t> cols((size_t)i + 1);
      std::iota(cols.begin(), cols.end(), 0);
      std::shuffle(cols.begin(), cols.end(), rng);
      for (int64_t k = 0; k < i; ++k) { t.row.push_back((int32_t)i); t.col.push_back(cols[(size_t)k]); t.val.push_back((double)k / 7.0); }
    }
    std::vector<size_t> p(t.val.size());
    std::iota(p.begin(), p.end(), (size_t)0);
    std::shuffle(p.begin(), p.end(), rng);
    Triples s;
    for (size_t q : p) { s.row.push_back(t.row[q]); s.col.push_back(t.col[q]); s.val.push_back(t.val[q]); }
    CHECK(coo_first_bad(n, (int64_t)s.val.size(), s.row.data(), s.col.data(), 0, true) == -1);
    check_row_form(n, s, 0);
    for (auto& r : s.row) r += 1;
    for (auto& c : s.col) c += 1;
    CHECK(coo_first_bad(n, (int64_t)s.val.size(), s.row.data(), s.col.data(), 1, true) == -1);
    check_row_form(n, s, 1);
  }
  // n = 1: no triple (null arrays), three duplicates; every triple in the last row
  {
    CooRowForm f;
    coo_row_form(1, 0, nullptr, nullptr, nullptr, 0, f);
    CHECK(f.row_ptr == std::vector<int64_t>({0, 0}) && f.perm.empty() && f.col.empty());
    CHECK(coo_first_bad(1, 0, nullptr, nullptr, 1, true) == -1);
    CHECK(coo_bad_arguments(1, 0, 0, 0, 3, nullptr, nullptr, nullptr, nullptr).empty());
    Triples three{{0, 0, 0}, {0, 0, 0}, {1.0, -1.0, 0x1p-60}};
    check_row_form(1, three, 0);
    Triples last;
    for (int k = 0; k < 200; ++k) { last.row.push_back(299); last.col.push_back((int32_t)((k * 37) % 300)); last.val.push_back(k); }
    CHECK(coo_first_bad(300, 200, last.row.data(), last.col.data(), 0, true) == -1);
    check_row_form(300, last, 0);
  }
  // refusals
  {
    const int64_t n = 500;
    Triples t;
    for (int k = 0; k < 3000; ++k) {
      const int32_t i = (int32_t)(rng() % n), j = (int32_t)(rng() % n);
      t.row.push_back(std::max(i, j)); t.col.push_back(std::min(i, j)); t.val.push_back(1.0);
    }
    auto first = [&](const Triples& x, int base, bool lower) { return coo_first_bad(n, (int64_t)x.val.size(), x.row.data(), x.col.data(), base, lower); };
    CHECK(first(t, 0, true) == -1);
    Triples x = t; x.row[17] = -1; CHECK(first(x, 0, false) == 17);
    x = t; x.row[17] = (int32_t)n; CHECK(first(x, 0, false) == 17);
    x = t; for (auto& r : x.row) r += 1; for (auto& c : x.col) c += 1; x.row[5] = 0; CHECK(first(x, 1, false) == 5);
    x = t; x.col[29] = (int32_t)n; CHECK(first(x, 0, false) == 29);
    x = t; x.col[1500] = (int32_t)n + 3; x.col[40] = -7; CHECK(first(x, 0, false) == 40);
    x = t; x.row[77] = 3; x.col[77] = 9; CHECK(first(x, 0, false) == -1 && first(x, 0, true) == 77);
    x = t; x.row[0] = INT32_MIN; x.col[1] = INT32_MAX; CHECK(first(x, 1, false) == 0);
    const int bits16[2] = {16, 32}, bits_ok[2] = {64, 32};
    const void* some = t.val.data();
    CHECK(coo_bad_arguments(n, -1, 0, 0, 3, nullptr, some, some, some) == "nnz = -1 must not be negative");
    CHECK(coo_bad_arguments(n, (int64_t)1 << 32, 0, 0, 3, nullptr, some, some, some).find("below 2^32") != std::string::npos);
    CHECK(coo_bad_arguments(n, 10, 0, 0, 3, nullptr, some, some, nullptr) == "null vals");
    CHECK(coo_bad_arguments(n, 10, 0, 0, 3, nullptr, nullptr, some, some) == "null row_idx");
    CHECK(coo_bad_arguments(n, 10, 2, 0, 3, nullptr, some, some, some) == "index_base must be 0 or 1");
    CHECK(coo_bad_arguments(n, 10, 0, 4, 3, nullptr, some, some, some) == "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER");
    CHECK(coo_bad_arguments(n, 10, 0, 3, 3, bits16, some, some, some) == "row_bits must be 32 or 64");
    CHECK(coo_bad_arguments(n, 10, 1, 3, 3, bits_ok, some, some, some).empty());
  }
  std::printf(failures ? "coo_driver: %d check(s) FAILED\n" : "coo_driver: ok\n", failures);
  return failures ? 1 : 0;
}
