// Drives pcgx::KDTree::Boundary (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_boundary.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n            followed by n lines "x y z nx ny nz"   the cloud (a tree over it) and one normal per point
//   B r gap minnb  Boundary(r, normals, gap, minnb)
// Output: per B four lines: "I id id ...", "G gap ...", "M mask ..." (decimal), "C count ...".
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
        for (size_t i = 0; i < n; i++)
          in >> pts[i][0] >> pts[i][1] >> pts[i][2] >> normals[i][0] >> normals[i][1] >> normals[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "B") {
        float r;
        int32_t gap, minnb;
        in >> r >> gap >> minnb;
        const auto res = tree->Boundary(r, normals, gap, minnb);
        std::printf("I");
        for (int64_t id : res.ids) std::printf(" %" PRId64, id);
        std::printf("\nG");
        for (int32_t g : res.gaps) std::printf(" %d", (int)g);
        std::printf("\nM");
        for (uint64_t m : res.masks) std::printf(" %" PRIu64, m);
        std::printf("\nC");
        for (int32_t c : res.counts) std::printf(" %d", (int)c);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
