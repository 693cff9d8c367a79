// isle_amd/host/resident_host_main.cpp — the ledger of what a context holds (../csrc/resident_host.h) driven by a script on stdin, one event
// per line, every field and predicate as one JSON object per line on stdout: no library, no GPU (tests/test_resident_host_cpu.py builds it
// with the address and undefined-behaviour sanitizers and states every expected field itself).
//   state 0|1            every flag false / true, every size 0 / 9, the form and the space -1 / 1, Pt2 absent / by position, the counters 0 / 5
//   set <field> <value>  one field (Pt2: 0 absent, 1 by document, 2 by position)
//   ask <k>              the k the predicates are asked with from here on (9 at the start)
//   <event> [args]       a member function of IsleResident by name; its arguments as integers
#include <cstdio>
#include <iostream>
#include <string>

#include "../csrc/resident_host.h"

namespace {

template <class T>
T take() {
  T v = T();
  std::cin >> v;
  return v;
}

void all(IsleResident& r, bool on) {
  r.a_ready = r.a_avg_valid = r.b_from_threshold = r.band_ready = r.P_ready = r.Pt_ready = r.centers_ready = r.lift_valid = r.assign_valid = r.members_valid = on;
  r.p_catch_ready = r.p_model_ready = r.p_avg_ready = r.ml_ready = r.inf_valid = on;
  r.U_k = r.kmpp_track_k = r.km_proj_k = r.centers_k = r.lift_ld = r.lift_k = r.km_last_k = r.p_k = on ? 9 : 0;
  r.gl_mode = r.km_last_space = on ? 1 : -1;
  r.Pt2 = on ? ISLE_PT2_BY_POSITION : ISLE_PT2_ABSENT;
  r.P_gen = r.kmpp_P_gen = r.km_proj_P_gen = on ? 5 : 0;
}

bool set(IsleResident& r, const std::string& f, long long v) {
#define B(name) if (f == #name) return r.name = v != 0, true
#define I(name) if (f == #name) return r.name = (int)v, true
#define G(name) if (f == #name) return r.name = (uint64_t)v, true
  B(a_ready); B(a_avg_valid); B(b_from_threshold); B(band_ready); B(P_ready); B(Pt_ready); B(centers_ready); B(lift_valid); B(assign_valid);
  B(members_valid); B(p_catch_ready); B(p_model_ready); B(p_avg_ready); B(ml_ready); B(inf_valid);
  I(gl_mode); I(U_k); I(kmpp_track_k); I(km_proj_k); I(centers_k); I(lift_ld); I(lift_k); I(km_last_space); I(km_last_k); I(p_k);
  G(P_gen); G(kmpp_P_gen); G(km_proj_P_gen);
#undef B
#undef I
#undef G
  if (f == "Pt2" && v >= 0 && v <= 2) return r.Pt2 = (IslePt2)v, true;
  return false;
}

bool event(IsleResident& r, const std::string& e) {
#define E0(name) if (e == #name) return r.name(), true
#define E1(name) if (e == #name) { const int a = take<int>(); return r.name(a), true; }
#define E1B(name) if (e == #name) { const int a = take<int>(); return r.name(a != 0), true; }
  E0(A_rewrite_begins); E0(A_installed); E0(corpus_average_known); E1B(B_replaced); E1B(operator_form_decided); E0(operator_built);
  E0(operator_must_be_rebuilt); E1(U_installed); E0(projection_begins); E1B(projection_made); E0(transposed_copy_made); E0(split_copy_made);
  E0(P_overwritten); E0(kmpp_begins); E1(kmpp_kept_first_assignment); E0(lloyd_projected_begins); E0(kmpp_first_assignment_taken);
  E0(partition_rewrite_begins); E1(centres_installed); E0(centres_not_lifted); E0(lloyd_word_begins); E0(member_lists_built);
  E0(member_lists_stale); E0(partition_given); E1(catchwords_done); E0(topic_model_done); E0(avg_model_begins); E0(avg_model_done);
  E0(model_loaded); E0(inference_begins); E0(inference_done);
#undef E0
#undef E1
#undef E1B
  if (e == "lloyd_projected_done") {
    const int space = take<int>(), k = take<int>();
    return r.lloyd_projected_done(space, k), true;
  }
  if (e == "centres_lifted") {
    const int ld = take<int>(), k = take<int>();
    return r.centres_lifted(ld, k), true;
  }
  if (e == "lloyd_word_done") {
    const int space = take<int>(), k = take<int>(), iterated = take<int>();
    return r.lloyd_word_done(space, k, iterated != 0), true;
  }
  return false;
}

void print(const IsleResident& r, const std::string& cmd, int k) {
  std::printf("{\"cmd\": \"%s\"", cmd.c_str());
#define P(name) std::printf(", \"" #name "\": %lld", (long long)r.name)
  P(a_ready); P(a_avg_valid); P(b_from_threshold); P(gl_mode); P(band_ready); P(U_k); P(P_ready); P(Pt_ready); P(Pt2); P(P_gen); P(kmpp_track_k);
  P(kmpp_P_gen); P(km_proj_k); P(km_proj_P_gen); P(centers_ready); P(centers_k); P(lift_valid); P(lift_ld); P(lift_k); P(assign_valid);
  P(km_last_space); P(km_last_k); P(members_valid); P(p_k); P(p_catch_ready); P(p_model_ready); P(p_avg_ready); P(ml_ready); P(inf_valid);
#undef P
  std::printf(", \"Pt2_ready\": %d, \"Pt2_by_position\": %d, \"kmpp_same_P\": %d, \"thin\": %d, \"part_word\": %d, \"part_proj\": %d, \"proj\": %d", (int)r.Pt2_ready(),
              (int)r.Pt2_by_position(), (int)r.kmpp_same_P(), (int)r.thin_product_possible(k), (int)r.loop_partition_resident(0, k, true),
              (int)r.loop_partition_resident(1, k, false), (int)r.loop_projection_resident());
  std::printf(", \"centres_word\": %d, \"centres_proj\": %d}\n", (int)r.loop_centres_resident(true, k), (int)r.loop_centres_resident(false, k));
}

}  // namespace

int main() {
  IsleResident r;
  int k = 9;
  std::string cmd;
  while (std::cin >> cmd) {
    bool ok = true;
    if (cmd == "state") {
      all(r, take<int>() != 0);
    } else if (cmd == "set") {
      const std::string f = take<std::string>();
      ok = set(r, f, take<long long>());
    } else if (cmd == "ask") {
      k = take<int>();
    } else {
      ok = event(r, cmd);
    }
    if (!ok || !std::cin) {
      std::fprintf(stderr, "resident_host_main: %s: unknown, or its arguments ended or did not parse\n", cmd.c_str());
      return 2;
    }
    print(r, cmd, k);
  }
  return 0;
}
