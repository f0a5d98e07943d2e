// tlassim — csrc/tlas_build.hpp's level-wise build of the top-level hierarchy against host_scene.hpp::buildTopLevel, byte for byte
// (tests/test_tlas_build_host.py).
//
//   tlassim SUITE
//
// SUITE is a file of tests/tlassuite.py::save: the words 'TLS1', number of cases; per case kind, leaf count, node count, the nodes'
// mesh words (int32) and their nodeWorld pairs (8 floats per node). Per case one line
//   EQUAL|DIFFERENT case K kind KIND leaves L nodes N records R height H
// and OK at the end if every case is EQUAL (exit status 0).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../yart_amd/csrc/host_scene.hpp"
#include "../../yart_amd/csrc/tlas_build.hpp"

using namespace yart_hip;

template <class T>
static bool readWords(std::FILE* f, T* out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: tlassim SUITE\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t head[2];
  if (!readWords(f, head, 2) || head[0] != 0x31534c54u) { std::fprintf(stderr, "not a suite file\n"); return 2; }
  int failures = 0;
  for (uint32_t k = 0; k < head[1]; k++) {
    uint32_t rec[3];
    if (!readWords(f, rec, 3)) { std::fprintf(stderr, "truncated\n"); return 2; }
    const uint32_t nn = rec[2];
    std::vector<int32_t> mesh(nn);
    std::vector<f4> world(size_t(nn) * 2u);
    if (!readWords(f, mesh.data(), nn) || !readWords(f, world.data(), size_t(nn) * 2u)) { std::fprintf(stderr, "truncated\n"); return 2; }
    std::vector<NodeDev> nodes(nn);
    for (uint32_t i = 0; i < nn; i++) nodes[i].mesh = mesh[i];
    std::vector<TlasNode> want, got;
    const uint32_t heightWant = buildTopLevel(nodes, world, want);
    const uint32_t heightGot = tlasBuildLevelwise(mesh.data(), nn, world.data(), got);
    const bool ok = heightWant == heightGot && want.size() == got.size() &&
                    (want.empty() || std::memcmp(want.data(), got.data(), want.size() * sizeof(TlasNode)) == 0);
    std::printf("%s case %u kind %u leaves %u nodes %u records %zu height %u\n", ok ? "EQUAL" : "DIFFERENT", k, rec[0], rec[1], nn, want.size(),
                heightWant);
    if (!ok) failures++;
  }
  std::fclose(f);
  if (failures) { std::printf("%d cases differ\n", failures); return 1; }
  std::printf("OK\n");
  return 0;
}
