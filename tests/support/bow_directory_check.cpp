// bow_directory_check.cpp -- stand-alone check of csrc/bow_directory.h (tests/test_keyframe_handles_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a child process).  argv[1] names a text file: n, then n nodes.  Prints three lines:
// order, nodes, first.
#include <cstdio>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/bow_directory.h"

static void line(const std::vector<int32_t>& v)
{
    for (size_t i = 0; i < v.size(); i++) std::printf(i ? " %d" : "%d", v[i]);
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    std::vector<int32_t> node(n);
    for (int i = 0; i < n; i++) if (std::fscanf(f, "%d", &node[i]) != 1) return 2;
    std::fclose(f);
    BowDirectory D;
    bow_directory_build(node.data(), n, D);
    line(D.order); line(D.nodes); line(D.first);
    return 0;
}
