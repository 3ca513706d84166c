// Drives pcgx::KDTree::FarthestPoints (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_fps.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n             followed by n lines "x y z"      the cloud (a tree over it)
//   Q count start   FarthestPoints at that count and start, with owners
// Output: per Q four lines: "K id ..." (the picks), "D bits ..." (dist_sq as hex words), "C bits" (cover_sq),
// "O owner ..." (one per point).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
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
      } else if (tag == "Q") {
        int64_t count, start;
        in >> count >> start;
        const auto res = tree->FarthestPoints(count, start, true);
        std::printf("K");
        for (int64_t id : res.ids) std::printf(" %" PRId64, id);
        std::printf("\nD");
        for (float d : res.distSq) std::printf(" %08" PRIx32, bits(d));
        std::printf("\nC %08" PRIx32 "\nO", bits(res.coverSq));
        for (int64_t id : res.owner) std::printf(" %" PRId64, id);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
