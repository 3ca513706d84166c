// Drives pcgx::KDTree::FPFH (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_fpfh.py compares
// with the Python binding's results.
// Input: a text file written by the test
//   P n   followed by n lines "x y z nx ny nz"   the cloud (a tree over it) and one normal per point
//   F r   FPFH(r, normals)
// Output: one line per point: 33 values (%.9g: float32 round trips exactly), 33 counts, the pair count.
#include <cinttypes>
#include <cstdio>
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
    std::vector<pcgx::Vec3> normals;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        normals.resize(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2] >> normals[i][0] >> normals[i][1] >> normals[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "F") {
        float r;
        in >> r;
        const auto res = tree->FPFH(r, normals);
        for (size_t i = 0; i < res.fpfh.size(); i++) {
          for (float v : res.fpfh[i]) std::printf("%.9g ", v);
          for (int32_t c : res.counts[i]) std::printf("%d ", (int)c);
          std::printf("%d\n", (int)res.pairs[i]);
        }
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
