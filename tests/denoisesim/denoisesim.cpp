// denoisesim.cpp — TEST INFRASTRUCTURE for tests/test_denoise.py, never part of libyart_hip.so.
//
// yart_amd/csrc/denoise.hpp's plain filter compiled as host C++ (as tests/hostsim and tests/aovsim compile the other device
// headers); the file format and the pass driver are dn_host.hpp, shared with tests/momentsim `denoisevar`.
//   denoisesim <in> <out>
#include "dn_host.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: denoisesim <in> <out>\n"); return 1; }
  try {
    dnHostRunFile<false>(argv[1], argv[2]);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "denoisesim: %s\n", e.what());
    return 2;
  }
}
