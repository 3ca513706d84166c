// Drives pcgx::KDTree::DBSCAN and pcgx::RadiusOutlierRemoval (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what
// tests/test_cpp_dbscan.py compares with the Python binding's results.
// Input: a text file written by the test
//   P n                              followed by n lines "x y z": the cloud (a tree over it)
//   D r minPts minSize maxSize       DBSCAN(...)
//   R r minNeighbors negative        RadiusOutlierRemoval(...).Filter over the cloud as 12-byte records
// Output per D: "L label ..." (one per point), "S size ..." (one per cluster), "I id ..." (the members, cluster by
// cluster), "K kind ..." (one per point), "M id ..." (Members of the last cluster); per R: "F x y z ..." (the kept
// records' coordinates as float32 bit patterns).
#include <cinttypes>
#include <cstdio>
#include <cstring>
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
    std::vector<pcgx::Vec3> pts;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        pts.resize(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "D") {
        float r;
        int min_pts;
        int64_t min_size, max_size;
        in >> r >> min_pts >> min_size >> max_size;
        const auto res = tree->DBSCAN(r, min_pts, min_size, max_size);
        line("L", res.labels);
        line("S", res.sizes);
        line("I", res.ids);
        line("K", std::vector<int64_t>(res.kind.begin(), res.kind.end()));
        line("M", res.sizes.empty() ? std::vector<int64_t>() : res.Members(res.sizes.size() - 1));
      } else if (tag == "R") {
        float r;
        int min_neighbors, negative;
        in >> r >> min_neighbors >> negative;
        const pcgx::CloudView view{pts.data(), (int64_t)pts.size(), 12, 0};
        const auto out = pcgx::RadiusOutlierRemoval(r, min_neighbors).WithNegative(negative != 0).Filter(view);
        std::vector<int64_t> bits(out.size() / 4);
        for (size_t k = 0; k < bits.size(); k++) {
          uint32_t b;
          std::memcpy(&b, out.data() + 4 * k, 4);
          bits[k] = b;
        }
        line("F", bits);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}
