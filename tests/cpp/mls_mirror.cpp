// Drives pcgx::KDTree::MLS (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_mls.py compares with
// the Python binding's results.
// Input: a text file written by the test
//   P n         followed by n lines "x y z"   the cloud (a tree over it)
//   M r s o k vx vy vz m  followed by m lines "x y z"   MLS(r, s, o, k, {vx, vy, vz}, queries); m == 0: the tree's own points
// Output: one line per result "px py pz nx ny nz kind count" (%.9g: float32 round trips exactly).
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
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "M") {
        float r, s;
        pcgx::Vec3 vp;
        int32_t o, k;
        size_t m;
        in >> r >> s >> o >> k >> vp[0] >> vp[1] >> vp[2] >> m;
        std::vector<pcgx::Vec3> q(m);
        for (auto &p : q) in >> p[0] >> p[1] >> p[2];
        const auto res = tree->MLS(r, s, o, k, vp, q);
        for (size_t i = 0; i < res.points.size(); i++)
          std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %d %d\n", res.points[i][0], res.points[i][1], res.points[i][2],
                      res.normals[i][0], res.normals[i][1], res.normals[i][2], (int)res.kinds[i], (int)res.counts[i]);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
