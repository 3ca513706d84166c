// Drives pcgx::KDTree::OrientNormals (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_orient.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n                 followed by n lines "x y z nx ny nz"   the cloud (a tree over it) and its normals
//   Q r mode rx ry rz   OrientNormals at that radius, mode 0 / 1 / 2 and direction or viewpoint
// Output: per Q three lines: "F flag ..." (one per point), "C component ..." (one per point), "N count" and then the
// normals' sign bits "S bit ..." (three per point).
#include <cinttypes>
#include <cmath>
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
        for (size_t i = 0; i < n; i++)
          in >> pts[i][0] >> pts[i][1] >> pts[i][2] >> normals[i][0] >> normals[i][1] >> normals[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "Q") {
        float r;
        int mode;
        pcgx::Vec3 ref;
        in >> r >> mode >> ref[0] >> ref[1] >> ref[2];
        const auto res = tree->OrientNormals(r, normals, (pcgx::KDTree::OrientMode)mode, ref);
        std::printf("F");
        for (uint8_t f : res.flipped) std::printf(" %d", (int)f);
        std::printf("\nC");
        for (int64_t c : res.component) std::printf(" %" PRId64, c);
        std::printf("\nN %" PRId64 "\nS", res.components);
        for (const auto &v : res.normals) std::printf(" %d %d %d", (int)std::signbit(v[0]), (int)std::signbit(v[1]), (int)std::signbit(v[2]));
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
