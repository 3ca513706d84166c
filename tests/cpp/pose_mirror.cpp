// Drives pcgx::pose_from_correspondences (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_pose.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n   followed by n lines "x y z"     the source points
//   Q n   followed by n lines "x y z"     the target points
//   C m   followed by m lines "src dst"   the pairs
//   U n   followed by n lines "u0 u1 u2"  the samples
//   E maxDist edgeSimilarity refine       one estimate: "E found best bestCount refined nInliers", the pose's sixteen
//                                         numbers on one line (%.9g: float32 round trips exactly), the inliers on one
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void read_points(std::ifstream &in, std::vector<pcgx::Vec3> &pts) {
  size_t n;
  in >> n;
  pts.resize(n);
  for (size_t i = 0; i < n; i++)
    for (float &v : pts[i]) {
      std::string w;  // (through strtof: operator>> refuses "inf" and "nan")
      in >> w;
      v = std::strtof(w.c_str(), nullptr);
    }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::vector<pcgx::Vec3> p, q;
    std::vector<std::array<int64_t, 2>> pairs;
    std::vector<std::array<uint32_t, 3>> samples;
    while (in >> tag) {
      if (tag == "P") {
        read_points(in, p);
      } else if (tag == "Q") {
        read_points(in, q);
      } else if (tag == "C") {
        size_t m;
        in >> m;
        pairs.resize(m);
        for (auto &c : pairs) in >> c[0] >> c[1];
      } else if (tag == "U") {
        size_t n;
        in >> n;
        samples.resize(n);
        for (auto &u : samples) in >> u[0] >> u[1] >> u[2];
      } else if (tag == "E") {
        float maxDist, es;
        int refine;
        in >> maxDist >> es >> refine;
        const auto r = pcgx::pose_from_correspondences(p, q, pairs, samples, maxDist, es, refine != 0);
        std::printf("E %d %" PRId64 " %" PRId64 " %d %zu\n", r.found ? 1 : 0, r.best, r.bestCount, r.refined ? 1 : 0,
                    r.inliers.size());
        for (float v : r.pose) std::printf("%.9g ", v);
        std::printf("\n");
        for (int64_t k : r.inliers) std::printf("%" PRId64 " ", k);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
