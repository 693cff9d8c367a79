"""isle_amd/csrc/resident_host.h, the ledger of what a context holds and which event voids it, without the library and without a GPU:
resident_host_main is built here with the address and undefined-behaviour sanitizers (a stand-alone program) and applies a script of events
that this file sends on stdin; it prints every field and predicate after every event.  What every event must leave is stated here as a
table, written event by event from the assignments the library made at its call sites before the ledger existed (the file and line of
that commit beside each row); nothing here reads the header, so no case can pass by agreement of the code with itself.

The split copy of the projection is one three-valued field here as there (0 absent, 1 by document, 2 by position): the two flags it
replaces were only ever read as "ready", and "by position" only where ready."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD, PROJECTED = 0, 1  # ISLE_SPACE_*

FLAGS = ("a_ready a_avg_valid b_from_threshold band_ready P_ready Pt_ready centers_ready lift_valid assign_valid members_valid p_catch_ready "
         "p_model_ready p_avg_ready ml_ready inf_valid").split()
SIZES = "U_k kmpp_track_k km_proj_k centers_k lift_ld lift_k km_last_k p_k".split()
GENS = "P_gen kmpp_P_gen km_proj_P_gen".split()
FIELDS = FLAGS + SIZES + GENS + ["gl_mode", "km_last_space", "Pt2"]


def state(on):
    """what `state 0|1` sets"""
    s = {f: int(on) for f in FLAGS}
    s.update({f: 9 if on else 0 for f in SIZES})
    s.update({f: 5 if on else 0 for f in GENS})
    s.update(gl_mode=1 if on else -1, km_last_space=1 if on else -1, Pt2=2 if on else 0)
    return s


def arg(i):
    return lambda s, a: a[i]


NO_PROJECTION = dict(P_ready=0, Pt_ready=0, Pt2=0)
NO_DOWNSTREAM = dict(p_catch_ready=0, p_model_ready=0, p_avg_ready=0)

# event -> (number of arguments, {field: value | f(state before, arguments)}); every field not named stays
EVENTS = {
    # api_stages.cpp:97,156,343 (ingest_tdf, feed_finalize, tdf_finalize) — and from this change on upload_counts_u32
    "A_rewrite_begins": (0, dict(a_ready=0)),
    # api_stages.cpp:34-35 install_A, api.cpp:560-569 isle_void_derived_from_A
    "A_installed": (0, dict(a_ready=1, a_avg_valid=0, inf_valid=0, **NO_DOWNSTREAM)),
    # api_stages.cpp:390 (thresholding), :587 (ensure_avg_doc_sz)
    "corpus_average_known": (0, dict(a_avg_valid=1)),
    # api.cpp:570-585 isle_void_derived_from_B, then :599 (upload: false) / api_stages.cpp:495 (thresholding: true)
    "B_replaced": (1, dict(band_ready=0, gl_mode=-1, lift_valid=0, members_valid=0, U_k=0, centers_ready=0, assign_valid=0, kmpp_track_k=0, km_last_space=-1,
                           km_proj_k=0, b_from_threshold=arg(0), **NO_PROJECTION, **NO_DOWNSTREAM)),
    # gram_lds.hip:1376 (0 before the device work), :1401 (flag ? 0 : 1)
    "operator_form_decided": (1, dict(gl_mode=arg(0))),
    "operator_built": (0, dict(band_ready=1)),             # spmm.hip:208
    "operator_must_be_rebuilt": (0, dict(band_ready=0)),   # api_ks.cpp:420
    # api_ks.cpp:368-373 install_U
    "U_installed": (1, dict(U_k=arg(0), lift_valid=0, centers_ready=0, **NO_PROJECTION)),
    # api_kmeans.cpp:56-58 ensure_P, behind `if (P_ready) return`
    "projection_begins": (0, dict(Pt_ready=0, Pt2=0)),
    # api_kmeans.cpp:66-70: P_ready, P_gen++, and with a2_done the split copy by position
    "projection_made": (1, dict(P_ready=1, P_gen=lambda s, a: s["P_gen"] + 1, Pt2=lambda s, a: 2 if a[0] else s["Pt2"])),
    "transposed_copy_made": (0, dict(Pt_ready=1)),         # dense.hip:1106 k_ensure_pt
    "split_copy_made": (0, dict(Pt2=1)),                   # api_kmeans.cpp:76, reached behind :58 only: by document
    # api_kmeans.cpp:710-712 (first assignment through the f32 product), spmm.hip:682-684 (wide product of the LDS form)
    "P_overwritten": (0, dict(**NO_PROJECTION)),
    "kmpp_begins": (0, dict(km_proj_k=0, kmpp_track_k=0)),  # api_kmeans.cpp:210,214
    # api_kmeans.cpp:268-269
    "kmpp_kept_first_assignment": (1, dict(kmpp_P_gen=lambda s, a: s["P_gen"], kmpp_track_k=arg(0))),
    "lloyd_projected_begins": (0, dict(km_proj_k=0, km_last_space=-1)),  # api_kmeans.cpp:531-532
    "partition_rewrite_begins": (0, dict(assign_valid=0)),               # api_kmeans.cpp:542, :894
    "kmpp_first_assignment_taken": (0, dict(kmpp_track_k=0)),            # api_kmeans.cpp:552
    # api_kmeans.cpp:582-585
    "lloyd_projected_done": (2, dict(km_last_space=arg(0), km_last_k=arg(1), km_proj_k=arg(1), km_proj_P_gen=lambda s, a: s["P_gen"])),
    "centres_installed": (1, dict(centers_ready=1, centers_k=arg(0))),   # api_kmeans.cpp:599-600
    "centres_lifted": (2, dict(lift_ld=arg(0), lift_k=arg(1), lift_valid=1)),  # api_kmeans.cpp:622-624
    "centres_not_lifted": (0, dict(lift_valid=0)),                       # api_kmeans.cpp:885, :908
    "lloyd_word_begins": (0, dict(km_last_space=-1)),                    # api_kmeans.cpp:878
    # api_kmeans.cpp:947-951: assign_valid always, the loop's space and k where max_reps > 0
    "lloyd_word_done": (3, dict(assign_valid=1, km_last_space=lambda s, a: a[0] if a[2] else s["km_last_space"],
                                km_last_k=lambda s, a: a[1] if a[2] else s["km_last_k"])),
    "member_lists_built": (0, dict(members_valid=1)),                    # kmeans.hip:1257, :1327
    "member_lists_stale": (0, dict(members_valid=0)),                    # api_kmeans.cpp:509, :853, :978
    "partition_given": (0, dict(assign_valid=1, members_valid=0, km_last_space=-1)),  # api_stages.cpp:659-661
    "catchwords_done": (1, dict(p_k=arg(0), p_catch_ready=1, p_model_ready=0, p_avg_ready=0)),  # api_stages.cpp:679-682
    "topic_model_done": (0, dict(p_model_ready=1)),                      # api_stages.cpp:711
    "avg_model_begins": (0, dict(p_avg_ready=0)),                        # api_stages.cpp:834
    "avg_model_done": (0, dict(p_avg_ready=1)),                          # api_stages.cpp:836
    "model_loaded": (0, dict(ml_ready=1)),                               # api_stages.cpp:986
    "inference_begins": (0, dict(inf_valid=0)),                          # infer_resident.hip:160
    "inference_done": (0, dict(inf_valid=1)),                            # infer_resident.hip:238
}


def predicates(s, k):
    """the tests the call sites spelt out: api_kmeans.cpp:375 (kmpp_same_P), :454 and kmeans.hip:314 (thin), :1029-1037 (the objective)"""
    return dict(
        Pt2_ready=int(s["Pt2"] != 0), Pt2_by_position=int(s["Pt2"] == 2),
        kmpp_same_P=int(s["kmpp_P_gen"] == s["P_gen"]),
        thin=int(s["gl_mode"] == 1 and bool(s["band_ready"]) and s["U_k"] == k),
        part_word=int(not (s["km_last_space"] != WORD or s["km_last_k"] != k or not s["assign_valid"])),
        part_proj=int(not (s["km_last_space"] != PROJECTED or s["km_last_k"] != k)),
        proj=int(not (not s["P_ready"] or s["P_gen"] != s["km_proj_P_gen"])),
        centres_word=int(not (not s["centers_ready"] or s["centers_k"] != k)),
        centres_proj=int(not (s["km_proj_k"] != k)))


def expect(script):
    """the table applied to the script: the line the program must print after every command"""
    s, k, out = state(False), 9, []
    for line in script:
        cmd, a = line[0], [int(x) for x in line[1:] if not isinstance(x, str)]
        if cmd == "state":
            s = state(a[0])
        elif cmd == "set":
            assert line[1] in FIELDS
            s[line[1]] = a[0]
        elif cmd == "ask":
            k = a[0]
        else:
            n, row = EVENTS[cmd]
            assert len(a) == n, line
            before = dict(s)
            for f, v in row.items():
                assert f in FIELDS, f
                s[f] = int(v(before, a)) if callable(v) else v
        out.append(dict(s, cmd=cmd, **predicates(s, k)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resident_host") / "resident_host_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "resident_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def run(exe, script):
    text = "\n".join(" ".join(str(t) for t in line) for line in script) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    return [json.loads(line) for line in r.stdout.splitlines()]


def check(exe, script):
    """every field and predicate after every command, against the table; -> the last line"""
    got, want = run(exe, script), expect(script)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys(), (i, script[i])
        diff = {f: (g[f], w[f]) for f in w if g[f] != w[f]}
        assert not diff, "after command %d %r: (printed, stated) %r" % (i, script[i], diff)
    return got[-1]


def calls(name):
    """the event with arguments that differ from both prepared states (9 / 0) and from each other"""
    if name in ("B_replaced", "operator_form_decided", "projection_made"):  # their argument is a yes or no
        return [[name, 0], [name, 1]]
    return [[name] + v for v in {0: [[]], 1: [[0], [1], [4]], 2: [[1, 4], [0, 6]], 3: [[0, 4, 1], [0, 4, 0], [1, 6, 1]]}[EVENTS[name][0]]]


# ---- every event alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EVENTS))
def test_every_event_alone_from_both_states(exe, name):
    for call in calls(name):
        for on in (0, 1):
            for gens in ([], [["set", "P_gen", 7]], [["set", "kmpp_P_gen", 3], ["set", "km_proj_P_gen", 4], ["set", "Pt2", 1]]):
                check(exe, [["state", on]] + gens + [["ask", 9], call, ["ask", 4], call, ["ask", 0], call])


def test_the_table_names_every_event_the_program_knows_and_no_other(exe):
    src = open(os.path.join(ROOT, "isle_amd", "host", "resident_host_main.cpp")).read()
    import re
    known = set(re.findall(r"E(?:0|1|1B)\((\w+)\);", src)) | set(re.findall(r'e == "(\w+)"', src))
    assert known == set(EVENTS)
    r = subprocess.run([exe], input="no_such_event\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unknown" in r.stderr
    r = subprocess.run([exe], input="set no_such_field 1\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---- sequences: the calls as the entries raise them ---------------------------------------------------------------------------------------
K = 4
UPLOAD_A = [["A_rewrite_begins"], ["A_installed"]]
THRESHOLD = [["corpus_average_known"], ["B_replaced", 1]]
SOLVE = [["operator_must_be_rebuilt"], ["operator_form_decided", 0], ["operator_form_decided", 1], ["operator_built"], ["U_installed", K]]
PROJECT_GROUPED = [["projection_begins"], ["projection_made", 1]]                                      # a large shard: the split copy by position on the way
PROJECT_PLAIN = [["projection_begins"], ["projection_made", 0], ["transposed_copy_made"]]              # a small one: the f32 transposed copy
PROJECT_SPLIT = PROJECT_PLAIN + [["split_copy_made"]]                                                  # a large one on another route
KMPP = [["kmpp_begins"], ["kmpp_kept_first_assignment", K]]
LLOYD_U = [["lloyd_projected_begins"], ["partition_rewrite_begins"], ["kmpp_first_assignment_taken"], ["member_lists_stale"], ["lloyd_projected_done", PROJECTED, K]]
LIFT = [["centres_installed", K], ["centres_lifted", K, K]]
LLOYD_B = [["lloyd_word_begins"], ["partition_rewrite_begins"], ["centres_not_lifted"], ["member_lists_built"], ["member_lists_stale"], ["lloyd_word_done", WORD, K, 1]]
POST = [["catchwords_done", K], ["topic_model_done"], ["avg_model_begins"], ["avg_model_done"]]
INFER = [["model_loaded"], ["inference_begins"], ["inference_done"]]
TRAINER = [["ask", K]] + UPLOAD_A + THRESHOLD + SOLVE + PROJECT_GROUPED + KMPP + LLOYD_U + LIFT + LLOYD_B + POST + INFER


def test_the_trainers_order_end_to_end(exe):
    s = check(exe, TRAINER)
    assert all(s[f] for f in FLAGS if f not in ("lift_valid", "members_valid", "Pt_ready"))
    assert (s["lift_valid"], s["members_valid"], s["Pt_ready"], s["Pt2"], s["kmpp_track_k"]) == (0, 0, 0, 2, 0)
    assert (s["km_last_space"], s["km_last_k"], s["km_proj_k"], s["centers_k"], s["p_k"], s["gl_mode"]) == (WORD, K, K, K, K, 1)
    assert (s["part_word"], s["part_proj"], s["proj"], s["centres_word"], s["centres_proj"], s["thin"]) == (1, 0, 1, 1, 1, 1)
    for project in (PROJECT_PLAIN, PROJECT_SPLIT):
        s = check(exe, [["ask", K]] + UPLOAD_A + THRESHOLD + SOLVE + project + KMPP + LLOYD_U)
        assert (s["P_ready"], s["Pt_ready"], s["Pt2"]) == (1, 1, 1 if project is PROJECT_SPLIT else 0)
        assert (s["part_proj"], s["proj"], s["centres_proj"], s["assign_valid"]) == (1, 1, 1, 0)


@pytest.mark.parametrize("k2", [K, 6])
def test_U_replaced_between_kmeanspp_and_lloyd(exe, k2):
    s = check(exe, TRAINER[:-len(LLOYD_U + LIFT + LLOYD_B + POST + INFER)] + [["U_installed", k2], ["ask", k2]])
    assert (s["U_k"], s["P_ready"], s["Pt2"], s["kmpp_track_k"], s["kmpp_same_P"]) == (k2, 0, 0, K, 1)  # kept, and the same P as far as anyone knows ...
    s = check(exe, TRAINER[:-len(LLOYD_U + LIFT + LLOYD_B + POST + INFER)] + [["U_installed", k2], ["ask", k2]] + PROJECT_GROUPED)
    assert (s["P_ready"], s["kmpp_track_k"], s["kmpp_same_P"]) == (1, K, 0)                             # ... until the new one is made: not taken


def test_P_overwritten_between_kmeanspp_and_lloyd(exe):
    head = [["ask", K]] + THRESHOLD + SOLVE + PROJECT_GROUPED + KMPP
    s = check(exe, head + [["P_overwritten"]])
    assert (s["P_ready"], s["Pt_ready"], s["Pt2"], s["kmpp_track_k"], s["kmpp_same_P"]) == (0, 0, 0, K, 1)
    s = check(exe, head + [["P_overwritten"]] + PROJECT_GROUPED)
    assert (s["P_ready"], s["Pt2"], s["kmpp_track_k"], s["kmpp_same_P"]) == (1, 2, K, 0)


def test_P_overwritten_between_lloyd_and_the_objectives_resident_form(exe):
    head = [["ask", K]] + THRESHOLD + SOLVE + PROJECT_PLAIN + KMPP + LLOYD_U
    assert check(exe, head)["proj"] == 1
    s = check(exe, head + [["P_overwritten"]])
    assert (s["part_proj"], s["centres_proj"], s["proj"]) == (1, 1, 0)
    s = check(exe, head + [["P_overwritten"]] + PROJECT_PLAIN)
    assert (s["P_ready"], s["part_proj"], s["centres_proj"], s["proj"]) == (1, 1, 1, 0)  # made again: not the one the loop ran on


def test_lloyd_twice_on_the_seeds_of_one_kmeanspp_call(exe):
    head = [["ask", K]] + THRESHOLD + SOLVE + PROJECT_GROUPED + KMPP
    s = check(exe, head + LLOYD_U[:2])
    assert (s["kmpp_track_k"], s["kmpp_same_P"], s["P_ready"]) == (K, 1, 1)  # where the route is chosen: the kept assignment is there
    s = check(exe, head + LLOYD_U + LLOYD_U[:2])
    assert (s["kmpp_track_k"], s["kmpp_same_P"], s["P_ready"]) == (0, 1, 1)  # the second time it is not
    s = check(exe, head + LLOYD_U + KMPP + LLOYD_U[:2])
    assert s["kmpp_track_k"] == K and s["km_proj_k"] == 0                    # a k-means++ call of its own: there again, and Cdev holds seeds


def test_B_replaced_after_everything(exe):
    for from_threshold in (0, 1):
        s = check(exe, TRAINER + [["B_replaced", from_threshold]])
        assert [f for f in FLAGS if s[f]] == ["a_ready", "a_avg_valid"] + (["b_from_threshold"] if from_threshold else []) + ["ml_ready", "inf_valid"]
        assert (s["U_k"], s["gl_mode"], s["Pt2"], s["km_last_space"], s["km_proj_k"], s["kmpp_track_k"]) == (0, -1, 0, -1, 0, 0)
        assert (s["thin"], s["part_word"], s["part_proj"], s["proj"], s["centres_word"], s["centres_proj"]) == (0, 0, 0, 0, 0, 0)


def test_A_rewritten_and_never_installed(exe):
    s = check(exe, TRAINER + [["A_rewrite_begins"]])
    assert s["a_ready"] == 0
    assert all(s[f] for f in ("a_avg_valid", "p_catch_ready", "p_model_ready", "p_avg_ready", "inf_valid", "assign_valid", "P_ready", "centers_ready"))
    s = check(exe, TRAINER + UPLOAD_A)
    assert [s[f] for f in ("a_ready", "a_avg_valid", "p_catch_ready", "p_model_ready", "p_avg_ready", "inf_valid", "ml_ready", "assign_valid")] == [1, 0, 0, 0, 0, 0, 1, 1]


def test_catchwords_for_another_k_after_a_topic_model(exe):
    s = check(exe, TRAINER + [["catchwords_done", 3]])
    assert (s["p_k"], s["p_catch_ready"], s["p_model_ready"], s["p_avg_ready"]) == (3, 1, 0, 0)
    s = check(exe, TRAINER + [["partition_given"], ["catchwords_done", K], ["topic_model_done"]])
    assert (s["assign_valid"], s["members_valid"], s["km_last_space"], s["part_word"], s["p_model_ready"], s["p_avg_ready"]) == (1, 0, -1, 0, 1, 0)


def test_member_lists_built_then_a_delta_update_of_the_sums(exe):
    s = check(exe, [["member_lists_built"], ["partition_rewrite_begins"], ["lloyd_word_done", WORD, K, 1], ["partition_given"], ["member_lists_built"]])
    assert s["members_valid"] == 1
    s = check(exe, [["member_lists_built"], ["partition_rewrite_begins"], ["lloyd_word_done", WORD, K, 1]])
    assert (s["members_valid"], s["assign_valid"]) == (1, 1)  # a new partition does not clear the lists: they are an order, not a result
    assert check(exe, [["member_lists_built"], ["member_lists_stale"]])["members_valid"] == 0
    assert check(exe, [["member_lists_built"], ["B_replaced", 0]])["members_valid"] == 0


def test_lloyd_without_an_iteration_leaves_no_loop_state(exe):
    s = check(exe, [["ask", K]] + THRESHOLD + SOLVE + PROJECT_PLAIN + LIFT + LLOYD_B[:-1] + [["lloyd_word_done", WORD, K, 0]])
    assert (s["assign_valid"], s["km_last_space"], s["part_word"]) == (1, -1, 0)
