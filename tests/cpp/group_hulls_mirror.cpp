// Drives pcgx::KDTree::GroupHulls (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_group_hulls.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n      followed by n lines "x y z": the cloud (a tree over it)
//   C r      Clusters(r), then GroupHulls of its result
// Output per C: "H hull_sizes ...", "I hull_ids ...", then "S" (area) and "R" (rect) with every value as the
// hexadecimal bits of a float64.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void ints(const char *tag, const std::vector<int64_t> &v) {
  std::printf("%s", tag);
  for (int64_t x : v) std::printf(" %" PRId64, x);
  std::printf("\n");
}

static void bits(const char *tag, const std::vector<double> &v) {
  std::printf("%s", tag);
  for (double d : v) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    std::printf(" %016" PRIx64, b);
  }
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::unique_ptr<pcgx::KDTree> tree;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "C") {
        float r;
        in >> r;
        const auto g = tree->GroupHulls(tree->Clusters(r));
        ints("H", g.hull_sizes);
        ints("I", g.hull_ids);
        bits("S", g.area);
        bits("R", g.rect);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
