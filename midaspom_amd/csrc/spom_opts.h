// midaspom_amd/csrc/spom_opts.h -- the one tokenizer of the "NAME=VALUE"
// option strings of the four _opts calls (mdp_engine_create_opts,
// mdp_future_create_opts, mdp_scenario_create_opts, mdp_scenario_sim_create).
// Each planner keeps its own table of names, defaults and messages.
#ifndef SPOM_OPTS_H
#define SPOM_OPTS_H
#include <string>

#include "mdp_internal.h"

// Pairs are separated by ';', ',', blank, tab or newline; empty tokens are
// skipped.  fn(key, value, has_value) is called once per pair in order: the
// text before the first '=', the text after it (empty without one), and
// whether there was one.  The first non-zero return ends the scan and is
// returned.  NULL is an empty string.
template <typename F>
int mdp_for_each_opt(const char *s, F &&fn)
{
    if (!s) return MDP_OK;
    std::string cur;
    for (const char *c = s;; ++c) {
        if (*c == 0 || *c == ';' || *c == ',' || *c == ' ' || *c == '\t' || *c == '\n') {
            if (!cur.empty()) {
                const size_t eq = cur.find('=');
                const bool has = eq != std::string::npos;
                const int rc = fn(cur.substr(0, eq), has ? cur.substr(eq + 1) : std::string(), has);
                if (rc) return rc;
                cur.clear();
            }
            if (*c == 0) break;
        } else {
            cur += *c;
        }
    }
    return MDP_OK;
}

#endif
