// Drives pcgx::score_poses and pcgx::pose_select (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_score.py compares with the Python binding's results.
// Input: a text file written by the test
//   T n   followed by n lines "x y z"     the tree's points
//   P n   followed by n lines "x y z"     the source points
//   M k   followed by k lines of sixteen  the poses (column-major)
//   S maxDist                             one scoring: "S best", the counts on one line, the sums (%.17g), the pose
//                                         (%.9g: float32 round trips exactly)
//   H n   followed by n lines "status count"   hypotheses (their poses: the M block's, one per hypothesis)
//   L K                                   one selection: "L selected", the ids on one line
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static float read_float(std::ifstream &in) {
  std::string w;  // (through strtof: operator>> refuses "inf" and "nan")
  in >> w;
  return std::strtof(w.c_str(), nullptr);
}

static void read_points(std::ifstream &in, std::vector<pcgx::Vec3> &pts) {
  size_t n;
  in >> n;
  pts.resize(n);
  for (size_t i = 0; i < n; i++)
    for (float &v : pts[i]) v = read_float(in);
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::vector<pcgx::Vec3> t, p;
    std::vector<pcgx::Mat4> poses;
    std::vector<int32_t> status;
    std::vector<int64_t> counts;
    std::unique_ptr<pcgx::KDTree> tree;
    while (in >> tag) {
      if (tag == "T") {
        read_points(in, t);
        tree.reset(new pcgx::KDTree(t));
      } else if (tag == "P") {
        read_points(in, p);
      } else if (tag == "M") {
        size_t k;
        in >> k;
        poses.resize(k);
        for (auto &m : poses)
          for (float &v : m) v = read_float(in);
      } else if (tag == "S") {
        const float maxDist = read_float(in);
        const auto r = pcgx::score_poses(*tree, p, poses, maxDist);
        std::printf("S %" PRId64 "\n", r.best);
        for (int64_t c : r.counts) std::printf("%" PRId64 " ", c);
        std::printf("\n");
        for (double s : r.sums) std::printf("%.17g ", s);
        std::printf("\n");
        for (float v : r.pose) std::printf("%.9g ", v);
        std::printf("\n");
      } else if (tag == "H") {
        size_t n;
        in >> n;
        status.resize(n);
        counts.resize(n);
        for (size_t h = 0; h < n; h++) in >> status[h] >> counts[h];
      } else if (tag == "L") {
        int64_t K;
        in >> K;
        const auto r = pcgx::pose_select(status, counts, poses, K);
        std::printf("L %" PRId64 "\n", r.selected);
        for (int64_t h : r.ids) std::printf("%" PRId64 " ", h);
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
