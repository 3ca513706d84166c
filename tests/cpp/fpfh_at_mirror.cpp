// Drives pcgx::KDTree::FPFHAt (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_fpfh_at.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n       followed by n lines "x y z nx ny nz"   the cloud (a tree over it) and one normal per point
//   A r k     followed by k ids                      FPFHAt(r, normals, ids)
// Output: one line per id: 33 values and the point's xyz (%.9g: float32 round trips exactly), 33 counts, the pair
// count; then one line "n_spfh <count>".
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
      } else if (tag == "A") {
        float r;
        size_t k;
        in >> r >> k;
        std::vector<int64_t> ids(k);
        for (size_t s = 0; s < k; s++) in >> ids[s];
        const auto res = tree->FPFHAt(r, normals, ids);
        for (size_t s = 0; s < res.fpfh.size(); s++) {
          for (float v : res.fpfh[s]) std::printf("%.9g ", v);
          for (float v : res.xyz[s]) std::printf("%.9g ", v);
          for (int32_t c : res.counts[s]) std::printf("%d ", (int)c);
          std::printf("%d\n", (int)res.pairs[s]);
        }
        std::printf("n_spfh %" PRId64 "\n", res.nSpfh);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
