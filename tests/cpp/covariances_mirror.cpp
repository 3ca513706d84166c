// Drives pcgx::KDTree::Covariances (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_covariances.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n                            followed by n lines "x y z"   the cloud (a tree over it)
//   C k r mode eps vx vy vz m      followed by m lines "x y z"   Covariances(k, r, mode, eps, queries, {vx, vy, vz});
//                                                                m == 0: the tree's own points
// Output: one line per query "count c0 .. c5 nx ny nz" (%.9g: float32 round trips exactly).
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
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "C") {
        int32_t k, mode;
        float r, eps;
        pcgx::Vec3 vp;
        size_t m;
        in >> k >> r >> mode >> eps >> vp[0] >> vp[1] >> vp[2] >> m;
        std::vector<pcgx::Vec3> q(m);
        for (auto &p : q) in >> p[0] >> p[1] >> p[2];
        const auto res = tree->Covariances(k, r, mode, eps, q, vp);
        for (size_t i = 0; i < res.cov.size(); i++) {
          std::printf("%d", (int)res.counts[i]);
          for (float c : res.cov[i]) std::printf(" %.9g", c);
          std::printf(" %.9g %.9g %.9g\n", res.normals[i][0], res.normals[i][1], res.normals[i][2]);
        }
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
