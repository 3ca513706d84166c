// Drives pcgx::KDTree::Clusters (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_clusters.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   P n                                 followed by n lines "x y z nx ny nz curvature": the cloud (a tree over it), one
//                                       normal and one curvature per point
//   C r useN minCos oriented useC maxCurvature minSize maxSize    Clusters(...), with the normals / the curvature or without
// Output per C: "L label ..." (one per point), "S size ..." (one per cluster), "I id ..." (the members, cluster by
// cluster), "M id ..." (Members of the last cluster).
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void line(const char *tag, const std::vector<int64_t> &v) {
  std::printf("%s", tag);
  for (int64_t x : v) std::printf(" %" PRId64, x);
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
    std::vector<pcgx::Vec3> normals;
    std::vector<float> curvature;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> pts(n);
        normals.resize(n);
        curvature.resize(n);
        for (size_t i = 0; i < n; i++)
          in >> pts[i][0] >> pts[i][1] >> pts[i][2] >> normals[i][0] >> normals[i][1] >> normals[i][2] >> curvature[i];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "C") {
        float r, min_cos, max_curvature;
        int use_n, oriented, use_c;
        int64_t min_size, max_size;
        in >> r >> use_n >> min_cos >> oriented >> use_c >> max_curvature >> min_size >> max_size;
        const auto res = tree->Clusters(r, use_n ? normals : std::vector<pcgx::Vec3>(), min_cos, oriented != 0,
                                        use_c ? curvature : std::vector<float>(), max_curvature, min_size, max_size);
        line("L", res.labels);
        line("S", res.sizes);
        line("I", res.ids);
        line("M", res.sizes.empty() ? std::vector<int64_t>() : res.Members(res.sizes.size() - 1));
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
