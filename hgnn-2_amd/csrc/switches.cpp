// The one reader of the HGNN_* kernel switches (host-only); switches.h holds the table and the parsing rules.
#include "switches.h"

#include <stdlib.h>
#include <string.h>

#include "../../include/hgnn_amd.h"

namespace hgnn {
namespace {
const char* env(const char* name) { const char* e = getenv(name); return e && e[0] ? e : nullptr; }  // empty = unset
void parse(const char* e, int dflt, int, int, bool& out) { out = e ? e[0] != '0' : dflt != 0; }
void parse(const char* e, int, int, int, Tri& out) { out = !e ? Tri::Auto : (e[0] == '0' ? Tri::Off : Tri::On); }
void parse(const char* e, int dflt, int lo, int hi, int& out) {
    char* end = nullptr;
    const long v = e ? strtol(e, &end, 10) : 0;
    out = e && !*end && v >= lo && v <= hi ? (int)v : dflt;
}

}  // namespace

const Switches& switches() {
    static const Switches once = [] {
        Switches s{};
#define X(type, field, name, dflt, lo, hi, what) parse(env(name), dflt, lo, hi, s.field);
        HGNN_SWITCH_TABLE(X)
#undef X
        s.dw_blocks_given = env("HGNN_DW_BLOCKS") != nullptr;
        return s;
    }();
    return once;
}
}  // namespace hgnn

extern "C" const char* hgnn_switch_name(int i) {
#define X(type, field, name, ...) name,
    static const char* const names[] = {HGNN_SWITCH_TABLE(X)};
#undef X
    return i >= 0 && i < (int)(sizeof(names) / sizeof(names[0])) ? names[i] : nullptr;
}

extern "C" int hgnn_switch_value(const char* name, int* value) {
    if (!name || !value) return HGNN_ERR_ARG;
    const hgnn::Switches& s = hgnn::switches();
#define X(type, field, variable, ...) if (!strcmp(name, variable)) return *value = (int)s.field, HGNN_OK;
    HGNN_SWITCH_TABLE(X)
#undef X
    return HGNN_ERR_ARG;
}
