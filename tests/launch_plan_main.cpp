// Stand-alone driver of csrc/launch_plan.h for tests/test_launch_plan_cpu.py: host compiler only, no HIP, no GPU.
// stdin, one case per line, fields separated by tabs:   KIND <tab> integer arguments, blank-separated <tab> NAME=value ...
// stdout, one line per case: the plan's description.  The switches come from the case's own table, never from the environment.
//   fwd   has_alpha has_touch
//   bwd   tiles has_depth has_alpha flags_min_r      (flags_min_r < 0: the switches' start value)
//   aside P late precomp has_sh debug
//   bins  tile_local tile_bits
//   ssim  gx gy planes
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "launch_plan.h"

static std::vector<std::pair<std::string, std::string>> g_table;
static const char* lookup(const char* name) {
  for (const auto& kv : g_table)
    if (kv.first == name) return kv.second.c_str();
  return nullptr;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<std::string> f;
    std::stringstream ls(line);
    for (std::string part; std::getline(ls, part, '\t');) f.push_back(part);
    if (f.size() < 2) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    g_table.clear();
    for (size_t i = 2; i < f.size(); i++) {
      const size_t eq = f[i].find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad switch: %s\n", f[i].c_str()); return 2; }
      g_table.emplace_back(f[i].substr(0, eq), f[i].substr(eq + 1));
    }
    long long a[5] = {0, 0, 0, 0, 0};
    std::stringstream as(f[1]);
    for (int i = 0; i < 5 && (as >> a[i]); i++) {}
    const GsrSwitches sw = gsr_switches_read(lookup);
    char d[160];
    if (f[0] == "fwd") gsr_plan_describe(gsr_plan_render_fwd(sw, a[0] != 0, a[1] != 0), d, sizeof d);
    else if (f[0] == "bwd") gsr_plan_describe(gsr_plan_render_bwd(sw, (int)a[0], a[1] != 0, a[2] != 0, a[3] < 0 ? sw.flags_min_r : (unsigned)a[3]), d, sizeof d);
    else if (f[0] == "aside") snprintf(d, sizeof d, "shade_aside=%d", gsr_plan_shade_aside(sw, (int)a[0], a[1] != 0, a[2] != 0, a[3] != 0, a[4] != 0));
    else if (f[0] == "bins") snprintf(d, sizeof d, "fused_bins=%d", gsr_plan_fused_bins(sw, a[0] != 0, (int)a[1]));
    else if (f[0] == "ssim") snprintf(d, sizeof d, "ssim_fwd tpw=%d", gsr_plan_ssim_tpw(sw, (int)a[0], (int)a[1], (int)a[2]));
    else { fprintf(stderr, "bad kind: %s\n", f[0].c_str()); return 2; }
    puts(d);
  }
  return 0;
}
