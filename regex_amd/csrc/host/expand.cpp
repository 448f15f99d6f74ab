// Replacement templates: expand.rs:50-91 (expand_bytes) and 127-166
// (find_cap_ref) restated, with the lookups that do not depend on the match
// (group names, group numbers past the regex's groups) done once.
#include "expand.hpp"

#include <cstring>

namespace rure_amd {

namespace {

// expand.rs:168-173 is_valid_cap_letter
bool cap_letter(uint8_t b) {
  return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z') || b == '_';
}

struct CapRef {
  bool number;
  uint32_t index;
  std::string name;
  size_t end;
};

// expand.rs:127-166: the reference at rep[0] == '$', false if there is none.
bool find_cap_ref(const uint8_t *rep, size_t n, CapRef *out) {
  if (n <= 1 || rep[0] != '$') return false;
  size_t i = 1;
  bool brace = false;
  if (rep[i] == '{') {
    brace = true;
    i = 2;
  }
  size_t end = i;
  while (end < n && cap_letter(rep[end])) ++end;
  if (end == i) return false;
  out->name.assign((const char *)rep + i, end - i);
  if (brace) {
    if (end >= n || rep[end] != '}') return false;
    ++end;
  }
  out->end = end;
  // cap.parse::<u32>(): decimal digits only, a value past u32 is a name
  uint64_t v = 0;
  out->number = true;
  for (char c : out->name) {
    if (c < '0' || c > '9') { out->number = false; break; }
    v = v * 10 + (uint64_t)(c - '0');
    if (v > 0xFFFFFFFFull) { out->number = false; break; }
  }
  out->index = (uint32_t)v;
  return true;
}

void push_lit(Template *t, const uint8_t *p, size_t n) {
  if (n == 0) return;
  if (!t->pieces.empty() && t->pieces.back().kind == 0) {
    t->pieces.back().b += (uint32_t)n;  // the pool is appended in order: adjacent literals are contiguous
  } else {
    t->pieces.push_back({0, (uint32_t)t->lits.size(), (uint32_t)n});
  }
  t->lits.append((const char *)p, n);
}

}  // namespace

Template compile_template(const uint8_t *rep, size_t rep_len, const std::vector<std::string> &names,
                          const std::vector<bool> &has_name) {
  Template t;
  const uint8_t dollar = '$';
  while (rep_len) {
    const uint8_t *d = (const uint8_t *)memchr(rep, '$', rep_len);
    if (!d) break;
    push_lit(&t, rep, (size_t)(d - rep));
    rep_len -= (size_t)(d - rep);
    rep = d;
    if (rep_len > 1 && rep[1] == '$') {
      push_lit(&t, &dollar, 1);
      rep += 2;
      rep_len -= 2;
      continue;
    }
    CapRef ref;
    if (!find_cap_ref(rep, rep_len, &ref)) {
      push_lit(&t, &dollar, 1);
      rep += 1;
      rep_len -= 1;
      continue;
    }
    rep += ref.end;
    rep_len -= ref.end;
    size_t g = names.size();
    if (ref.number) {
      g = ref.index;
    } else {
      for (size_t i = 0; i < names.size(); ++i)
        if (has_name[i] && names[i] == ref.name) { g = i; break; }
    }
    if (g >= names.size()) continue;  // expands to nothing for every match
    t.pieces.push_back({1, (uint32_t)g, 0});
    if (g != 0) t.names_groups = true;
  }
  push_lit(&t, rep, rep_len);
  return t;
}

}  // namespace rure_amd
