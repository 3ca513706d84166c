// Drives pcgx::fpfh_match / pcgx::fpfh_correspondences (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_match.py compares with the Python binding's results.
// Input: a text file written by the test
//   A n   followed by n lines of 33 values   the query rows
//   B n   followed by n lines of 33 values   the candidate rows
//   M     Match(A, B): one line per row of A: "M id distSq secondDistSq" (%.9g: float32 round trips exactly)
//   C r m Correspondences(A, B, r, m != 0): "C n", then one line "src dst" per pair
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void read_rows(std::ifstream &in, std::vector<pcgx::FPFHRow> &rows) {
  size_t n;
  in >> n;
  rows.resize(n);
  for (size_t i = 0; i < n; i++)
    for (float &v : rows[i]) {
      std::string w;  // (through strtof: operator>> refuses "inf" and "nan")
      in >> w;
      v = std::strtof(w.c_str(), nullptr);
    }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::vector<pcgx::FPFHRow> a, b;
    while (in >> tag) {
      if (tag == "A") {
        read_rows(in, a);
      } else if (tag == "B") {
        read_rows(in, b);
      } else if (tag == "M") {
        const auto r = pcgx::fpfh_match(a, b);
        for (size_t i = 0; i < r.ids.size(); i++)
          std::printf("M %" PRId64 " %.9g %.9g\n", r.ids[i], r.distSq[i], r.secondDistSq[i]);
      } else if (tag == "C") {
        float ratio;
        int mutual;
        in >> ratio >> mutual;
        const auto c = pcgx::fpfh_correspondences(a, b, ratio, mutual != 0);
        std::printf("C %zu\n", c.size());
        for (const auto &p : c) std::printf("%" PRId64 " %" PRId64 "\n", p[0], p[1]);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
