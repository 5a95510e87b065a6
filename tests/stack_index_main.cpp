// Drives serl_amd/csrc/stack_index.h (the index arithmetic of the fused gather + crop for frame stacks, no HIP) from a line
// protocol, one answer line per command, so tests/test_stack_index_cpu.py can compare it with NumPy on the CPU under the host
// sanitizers.  The program also does what the kernels do with the numbers: it writes one byte per (destination frame, part) and
// reads the crop table and the packed window at the computed places, so an index out of range is an AddressSanitizer report.
//   jobs <parts> <T> <batch> <n_cam>   -> jobs <part>:<t>:<i>:<cam>:<which>:<dst>:<crop>:<packed> ... (one per workgroup)
//   window <idx> <T> <cap>             -> window <slot of frame 0> ... <slot of frame T>
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "stack_index.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "jobs") {
      int parts, T, batch, n_cam;
      in >> parts >> T >> batch >> n_cam;
      const int64_t n = serl::stack_frame_blocks(parts, T, batch, n_cam);
      std::vector<uint8_t> out((size_t)2 * n_cam * batch * T * parts, 0);      // out_frames, one byte per part
      std::vector<int32_t> crop((size_t)batch * T * 2, 4);                     // the crop table
      std::vector<uint8_t> packed((size_t)batch * (T + 1), 1);                 // a packed window, one byte per frame
      std::cout << "jobs";
      long sum = 0;
      for (int64_t bid = 0; bid < n; ++bid) {
        const serl::StackJob j = serl::stack_job((int)bid, parts, T, batch, n_cam);
        const int64_t dst = serl::stack_dst_frame(j, T, batch, n_cam);
        const int ce = serl::stack_crop_entry(j, T);
        const int64_t pf = serl::stack_packed_frame(j, T);
        out[(size_t)dst * parts + j.part] += 1;
        sum += crop[(size_t)2 * ce] + crop[(size_t)2 * ce + 1] + packed[(size_t)pf];
        std::cout << ' ' << j.part << ':' << j.t << ':' << j.i << ':' << j.cam << ':' << j.which << ':' << dst << ':' << ce << ':' << pf;
      }
      bool once = sum == 9 * n;
      for (uint8_t v : out) once = once && v == 1;      // every (frame, part) of the output is written exactly once
      std::cout << (once ? " once" : " NOT-once") << std::endl;
    } else if (cmd == "window") {
      long long idx, cap;
      int T;
      in >> idx >> T >> cap;
      std::vector<uint8_t> ring((size_t)cap, 0);
      std::cout << "window";
      for (int f = 0; f <= T; ++f) {
        const int64_t s = serl::window_slot(idx, T, cap, f);
        ring[(size_t)s] += 1;
        std::cout << ' ' << (long long)s;
      }
      std::cout << std::endl;
    } else {
      std::cout << "error unknown command" << std::endl;
    }
  }
  return 0;
}
