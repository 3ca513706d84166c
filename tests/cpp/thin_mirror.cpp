// Drives pcgx::KDTree::Thin (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_thin.py compares
// with the Python binding's results.
// Input: a text file written by the test
//   P n           followed by n lines "x y z"      the cloud (a tree over it)
//   S m           followed by m scores             m = 0: hash mode from here on, else one score per point
//   Q r seed      Thin at that radius and seed, with owners
// Output: per Q two lines: "K id ..." (the kept ids), "O owner ..." (one per point).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::unique_ptr<pcgx::KDTree> tree;
    std::vector<float> score;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "S") {
        size_t m;
        in >> m;
        score.assign(m, 0.0f);
        for (size_t i = 0; i < m; i++) {  // (strtof: the stream's own extraction knows no "nan")
          std::string w;
          in >> w;
          score[i] = std::strtof(w.c_str(), nullptr);
        }
      } else if (tag == "Q") {
        float r;
        uint32_t seed;
        in >> r >> seed;
        const auto res = tree->Thin(r, seed, score, true);
        std::printf("K");
        for (int64_t id : res.ids) std::printf(" %" PRId64, id);
        std::printf("\nO");
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
