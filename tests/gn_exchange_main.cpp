// Drives serl_amd/csrc/gn_exchange.h (the bookkeeping of the fused GroupNorm epilogues' statistics exchange, no HIP) from a line
// protocol, one answer line per command, so tests/test_gn_exchange_cpu.py can compare it with NumPy on the CPU under the host
// sanitizers.  The program also does what the kernels do with the numbers: every tile of a launch writes its record and reads its
// peers' at the computed places in a region sized by gnx_records_per_image, so an index out of range is an AddressSanitizer report.
//   epoch <previous>                       -> epoch <next> <1 if the records must be zeroed first>
//   granule <value bits> <tag>             -> granule <value bits> <tag> (packed and unpacked again)
//   capacity <P> <Cout>                    -> capacity <records per image>
//   launch <images> <P> <Cout> <tile rows> <tile columns> <epoch>
//                                          -> launch <first>:<stride>:<count>:<self> ... (one per tile) <complete | INCOMPLETE>
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gn_exchange.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "epoch") {
      unsigned long long prev;
      in >> prev;
      const serl::GnxEpoch e = serl::gnx_next_epoch((uint32_t)prev);
      std::cout << "epoch " << e.epoch << ' ' << (e.clear ? 1 : 0) << std::endl;
    } else if (cmd == "granule") {
      unsigned long long v, t;
      in >> v >> t;
      const uint64_t g = serl::gnx_pack((uint32_t)v, (uint32_t)t);
      std::cout << "granule " << serl::gnx_value(g) << ' ' << serl::gnx_tag(g) << std::endl;
    } else if (cmd == "capacity") {
      int P, Cout;
      in >> P >> Cout;
      std::cout << "capacity " << serl::gnx_records_per_image(P, Cout) << std::endl;
    } else if (cmd == "launch") {
      int images, P, Cout, trows, tcols;
      unsigned long long epoch;
      in >> images >> P >> Cout >> trows >> tcols >> epoch;
      const int rows = P / trows, tiles_n = Cout / tcols;
      const long ntiles = (long)images * rows * tiles_n;
      // the layer's region as the workspace sizes it; tag 0 everywhere = zeroed before the first pass
      std::vector<uint64_t> rec((size_t)images * serl::gnx_records_per_image(P, Cout) * serl::kGnxGranules, 0);
      for (long t = 0; t < ntiles; ++t)   // publish: granule g of tile t carries the value t * 32 + g
        for (int g = 0; g < serl::kGnxGranules; ++g)
          rec[(size_t)t * serl::kGnxGranules + g] = serl::gnx_pack((uint32_t)(t * serl::kGnxGranules + g), (uint32_t)epoch);
      std::cout << "launch";
      bool complete = true;
      for (long t = 0; t < ntiles; ++t) {
        const serl::GnxPeers p = serl::gnx_peers(t, rows, tiles_n);
        std::cout << ' ' << p.first << ':' << p.stride << ':' << p.count << ':' << p.self;
        for (int k = 0; k < p.count; ++k) {   // collect: every peer's every granule is this pass's and is that peer's own value
          const long peer = p.first + (long)k * p.stride;
          for (int g = 0; g < serl::kGnxGranules; ++g) {
            const uint64_t x = rec[(size_t)peer * serl::kGnxGranules + g];
            complete = complete && serl::gnx_tag(x) == (uint32_t)epoch && serl::gnx_value(x) == (uint32_t)(peer * serl::kGnxGranules + g);
          }
        }
      }
      std::cout << (complete ? " complete" : " INCOMPLETE") << std::endl;
    } else {
      std::cout << "error unknown command" << std::endl;
    }
  }
  return 0;
}
