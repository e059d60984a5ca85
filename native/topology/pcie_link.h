// pcie_link — the negotiated PCIe link of one device, from sysfs.
//
// A link that trained at x8 or Gen4 instead of Gen5 x16 is a common fault on
// a freshly racked node and is invisible to every on-device test. This
// reads, and only reads, under <root>/bus/pci/devices/<bdf>/:
//   current_link_speed  max_link_speed    e.g. "32.0 GT/s PCIe"
//   current_link_width  max_link_width    e.g. "16"
// plus, for mi-hostlink, numa_node and pcie_replay_count in the same
// directory. A missing or unparsable file reads as unknown (-1), never as
// an error and never as a healthy link. No GPU or ROCm userspace needed;
// the root is injectable for fixture trees.

#pragma once

#include <string>

namespace k3samd {

struct PcieLink {
  double cur_gts = -1, max_gts = -1;  // GT/s per lane
  int cur_width = -1, max_width = -1;
  int gen = -1, max_gen = -1;  // 1..6 from the GT/s figure
  // GT/s x width / 8 x encoding (8b/10b for Gen1-2, 128b/130b from Gen3):
  // the payload rate before packet overhead. -1 when unknown.
  double raw_gbps = -1;
  bool known = false;     // current speed and width were both read
  bool degraded = false;  // current < max on either axis (needs both known)
};

PcieLink read_pcie_link(const std::string& sysfs_root, const std::string& bdf);

// One integer file of the device directory (numa_node, pcie_replay_count);
// `missing` when absent or unparsable.
long read_pcie_device_long(const std::string& sysfs_root,
                           const std::string& bdf, const std::string& name,
                           long missing);

// The fields as JSON members without braces: "link_known": .., "link_gen":
// .., "link_width": .., "link_max_gen": .., "link_max_width": ..,
// "link_raw_gbps": .., "link_degraded": ..
std::string pcie_link_json_members(const PcieLink& l);

}  // namespace k3samd
