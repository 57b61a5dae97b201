// The engine options' globals and stts_set_option / stts_get_option, all from the list in options.h.
#include "options.h"

#include <limits.h>

#include "../../include/stts2.h"

#define STTS_OPT_DEFINE(key, var, def, rule, lo, hi, fallback) int var = def;
STTS_OPTIONS(STTS_OPT_DEFINE)
#undef STTS_OPT_DEFINE

namespace {

struct Opt {
  int key, *var, rule, lo, hi, fallback;
};
#define STTS_OPT_ROW(key, var, def, rule, lo, hi, fallback) {key, &var, rule, lo, hi, fallback},
const Opt kOpts[] = {STTS_OPTIONS(STTS_OPT_ROW)};
#undef STTS_OPT_ROW

const Opt* find_opt(int key) {
  for (const Opt& o : kOpts)
    if (o.key == key) return &o;
  return nullptr;  // (unknown and retired keys)
}

}  // namespace

extern "C" {

int stts_set_option(int key, int value) {
  const Opt* o = find_opt(key);
  if (!o) return STTS_EINVAL;
  switch (o->rule) {
    case OPT_BOOL: *o->var = value != 0; break;
    case OPT_RAW: *o->var = value; break;
    case OPT_RANGE: *o->var = (value >= o->lo && value <= o->hi) ? value : o->fallback; break;
    case OPT_MIN0:
      if (value < 0) return STTS_EINVAL;
      *o->var = value;
      break;
  }
  return 0;
}

int stts_get_option(int key) {
  const Opt* o = find_opt(key);
  return o ? *o->var : STTS_EINVAL;
}

}  // extern "C"
