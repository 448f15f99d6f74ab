// The replacement template of bytes::Regex::replace* (expand.rs:50-166)
// compiled against a regex's capture groups, for the device expansion
// (kernels/expand_scan.hip).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace rure_amd {

struct TemplatePiece {
  uint32_t kind;  // 0: lits[a .. a + b), 1: group a (b = 0)
  uint32_t a, b;
};

struct Template {
  std::vector<TemplatePiece> pieces;
  std::string lits;          // the literal pool, never longer than the template
  bool names_groups = false; // some piece is a group other than 0
};

// names[i] = the name of group i ("" with has_name[i] false for an unnamed
// group).  References that expand to nothing for every match (an unknown
// name, a number >= the group count) are dropped, adjacent literals merged.
Template compile_template(const uint8_t *rep, size_t rep_len, const std::vector<std::string> &names,
                          const std::vector<bool> &has_name);

}  // namespace rure_amd
