#include "pcie_link.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>

namespace k3samd {
namespace {

std::string device_dir(const std::string& root, const std::string& bdf) {
  return root + "/bus/pci/devices/" + bdf + "/";
}

// First line of a file, "" when it cannot be read.
std::string first_line(const std::string& path) {
  std::ifstream f(path);
  std::string line;
  if (f) std::getline(f, line);
  return line;
}

// Leading number of "32.0 GT/s PCIe" / "16"; -1 for "", "Unknown", "0".
double leading_number(const std::string& s) {
  char* end = nullptr;
  const double v = std::strtod(s.c_str(), &end);
  return end == s.c_str() || v <= 0 ? -1 : v;
}

int gen_of(double gts) {
  static const double kRates[] = {2.5, 5, 8, 16, 32, 64};
  for (int g = 0; g < 6; ++g)
    if (gts > kRates[g] - 0.01 && gts < kRates[g] + 0.01) return g + 1;
  return -1;
}

}  // namespace

PcieLink read_pcie_link(const std::string& sysfs_root,
                        const std::string& bdf) {
  const std::string dir = device_dir(sysfs_root, bdf);
  PcieLink l;
  l.cur_gts = leading_number(first_line(dir + "current_link_speed"));
  l.max_gts = leading_number(first_line(dir + "max_link_speed"));
  l.cur_width = (int)leading_number(first_line(dir + "current_link_width"));
  l.max_width = (int)leading_number(first_line(dir + "max_link_width"));
  l.gen = l.cur_gts > 0 ? gen_of(l.cur_gts) : -1;
  l.max_gen = l.max_gts > 0 ? gen_of(l.max_gts) : -1;
  l.known = l.cur_gts > 0 && l.cur_width > 0;
  if (l.known) {
    const double encoding = l.cur_gts < 7.9 ? 8.0 / 10.0 : 128.0 / 130.0;
    l.raw_gbps = l.cur_gts * l.cur_width / 8.0 * encoding;
  }
  l.degraded = l.known && ((l.max_gts > 0 && l.cur_gts < l.max_gts - 0.01) ||
                           (l.max_width > 0 && l.cur_width < l.max_width));
  return l;
}

long read_pcie_device_long(const std::string& sysfs_root,
                           const std::string& bdf, const std::string& name,
                           long missing) {
  const std::string s = first_line(device_dir(sysfs_root, bdf) + name);
  char* end = nullptr;
  const long v = std::strtol(s.c_str(), &end, 10);
  return end == s.c_str() ? missing : v;
}

std::string pcie_link_json_members(const PcieLink& l) {
  char buf[256];
  std::snprintf(buf, sizeof(buf),
                "\"link_known\": %s, \"link_gen\": %d, \"link_width\": %d, "
                "\"link_max_gen\": %d, \"link_max_width\": %d, "
                "\"link_raw_gbps\": %.1f, \"link_degraded\": %s",
                l.known ? "true" : "false", l.gen, l.cur_width, l.max_gen,
                l.max_width, l.raw_gbps, l.degraded ? "true" : "false");
  return buf;
}

}  // namespace k3samd
