"""The cases and the certificate of inference and the document reports on document shards (tests/doc_shard_cases.py), without a GPU:
the corpus and the layouts hit what they are meant to hit, the certificate accepts per-rank results cut from the single-rank reference
and refuses results made by each wrong rule a sharded implementation could take, and the slice rule of isle_amd/csrc/stage_host.h
(topic_sums_slice) equals its Python restatement, through a stand-alone host program built here with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import doc_shard_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = tuple(l for l in dc.LAYOUTS if dc.WORLD[l] > 1)


# ---- the corpus and the layouts ---------------------------------------------------------------------------------------------------------
def test_the_corpus_is_what_it_should_be():
    case, R = dc.corpus(), dc.reference()
    lens = np.diff(case["offs"])
    assert len(lens) == dc.D == 2301 and case["V"] == 200 and case["topics"] == 7
    assert lens[50] == 0 and (lens[dc.EMPTY_RUN[0]:dc.EMPTY_RUN[1]] == 0).all() and dc.EMPTY_RUN[1] - dc.EMPTY_RUN[0] > dc.IT_WIN
    assert lens[dc.EMPTY_RUN[0] - 1] > 0 and lens[dc.EMPTY_RUN[1]] > 0
    ct, dts = R["catch_topic"], R["dts"]
    assert len(set(ct[ct >= 0].tolist())) == 7                                # every topic has catchwords
    assert (dts["top2"] >= 0).sum() > 1000 and ((dts["top1"] < 0) & (lens > 0)).any() is not None
    # the identical documents: bit-equal sums of the topics 3 and 5 in every one of them
    a, b = dc.TIES
    per = np.diff(dts["dts_off"])[a:b]
    assert (per == 2).all()
    o = dts["dts_off"][a]
    t, v = dts["dts_topic"][o:o + 2 * (b - a)].reshape(-1, 2), dts["dts_val"][o:o + 2 * (b - a)].view(np.uint32).reshape(-1, 2)
    assert (t == [3, 5]).all() and (v == v[0]).all()
    # the printed digits: documents 8 | 9, 98 | 99 and 998 | 999 print lines of every kind on both sides of 9 -> 10, 99 -> 100, 999 -> 1000
    for d in (8, 9, 98, 99, 998, 999):
        assert per[d - a] > 0 if a <= d < b else np.diff(dts["dts_off"])[d] > 0, d
        assert dts["top1"][d] >= 0 and dts["top2"][d] >= 0, d
        assert (ct[case["rows"][case["offs"][d]:case["offs"][d + 1]]] >= 0).any(), d


@pytest.mark.parametrize("layout", MULTI)
def test_layouts_hit_what_they_are_meant_to(layout):
    f = dc.layout_facts(layout)
    assert f["L"] % f["W"] != 0, f                                            # the slices are uneven
    assert sum(f["own"]) == f["L"] and f["few_L"] == 2
    assert f["avg"] not in [a for a, o in zip(f["shard_avgs"], f["own"]) if o] and f["avg"] != int(f["mean_of_shard_avgs"]), f
    if layout == "H2":
        assert min(f["slice_len"]) > dc.MT_TILE, f                            # a slice longer than one tile
        assert all(n >= 2 for n in f["tiles"]["catchwords"]) and f["tiles"]["topic_sums_by_doc"][0] >= 2 and min(f["tiles"]["top_two"]) >= 2
        assert all(f["cut_inside_tile"][k][0] for k in f["cut_inside_tile"]), f
        assert f["few_L"] == f["W"]
    else:
        assert f["few_L"] < f["W"]                                            # L < W
    if layout in ("E3", "E4"):
        assert 0 in f["own"] and max(f["own"]) > 0                            # a rank without sums beside the one with nmax
    if layout in ("E4", "C4"):
        assert f["cut_in_ties"], f                                           # a slice boundary inside a run of ties from two ranks, inside a topic
    if layout == "C4":
        assert list(dc.bounds(layout)[1:4]) == [8, 98, 998]


def test_the_small_ranges():
    for layout in MULTI:
        want = dc.expected_reports(layout)
        assert sum(len(p) for p in want["few"]) > 0 and sum(p.count(b"\n") for p in want["few"]) == 2
        assert all(p == b"" for p in want["none"])
        held = [dc.none_local(layout, q) for q in range(dc.WORLD[layout])]
        assert sum(e - b for b, e in held) == dc.EMPTY_RUN[1] - dc.EMPTY_RUN[0]


# ---- the certificate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_the_certificate_accepts_the_reference(layout):
    ranks = dc.reference_ranks(layout)
    assert dc.certify_reports(layout, ranks) == {k: "bytes equal" for k in dc.KINDS + ("few", "none")}
    dc.certify_avg(layout, ranks, "avg_th")
    want = dc.expected_reports(layout)
    R, case = dc.reference(), dc.corpus()
    from test_doc_report_cpu import catchwords_text, top_two_text, topic_sums_text
    dts = R["dts"]
    assert b"".join(want["catchwords"]) == catchwords_text(R["catch_topic"], case["offs"], case["rows"], case["nv"])
    assert b"".join(want["topic_sums"]) == topic_sums_text(dts["dts_off"], dts["dts_topic"], dts["dts_val"])
    assert b"".join(want["topic_sums_by_doc"]) == topic_sums_text(dts["dts_off"], dts["dts_topic"], dts["dts_val"], by_doc=True)
    assert b"".join(want["top_two"]) == top_two_text(dts["top1"], dts["top2"])


WRONG = [(l, w) for l in MULTI for w in ("local_numbers", "sort_per_shard", "slice_drop", "slice_repeat")] + [(l, "tie_order") for l in ("E4", "C4")]


@pytest.mark.parametrize("layout,wrong", WRONG)
def test_the_certificate_refuses_each_wrong_rule(layout, wrong):
    """tie_order on the layouts whose cut lies inside the identical documents: equal pairs on two ranks"""
    with pytest.raises(AssertionError, match="line \\d+: got|nbytes, nlines"):
        dc.certify_reports(layout, dc.reference_ranks(layout, wrong=wrong))


@pytest.mark.parametrize("layout", MULTI)
def test_the_certificate_refuses_the_average_of_one_shard(layout):
    ranks = dc.reference_ranks(layout, wrong="shard_avg")
    dc.certify_reports(layout, ranks)
    with pytest.raises(AssertionError, match="the corpus has"):
        dc.certify_avg(layout, ranks, "avg_th")


def test_the_inference_certificate():
    single = dc.fake_single()
    for layout in dc.LAYOUTS:
        assert dc.certify_infer(layout, dc.infer_ranks(layout, single, "inf"), single, "inf") == "bits equal"
        assert dc.certify_infer(layout, dc.infer_ranks(layout, single, "in", inner=True), single, "in", inner=True) == "bits equal"
    other = dc.fake_single(seed=6)
    with pytest.raises(AssertionError):
        dc.certify_infer("H2", dc.infer_ranks("H2", other, "inf"), single, "inf")
    with pytest.raises(AssertionError, match="text entries: line 1: got"):  # rows numbered from the shard's 0
        dc.certify_infer("C4", dc.infer_ranks("C4", single, "inf", local_numbers=True), single, "inf")
    flipped = dict(single, weight=single["weight"].copy())
    flipped["weight"].view(np.uint32)[-1] ^= 1  # one bit of the last rank's last entry
    with pytest.raises(AssertionError, match="weight differs in its bits"):
        dc.certify_infer("H2", dc.infer_ranks("H2", flipped, "inf"), single, "inf")


def test_first_difference_names_the_line():
    assert dc.first_difference(b"1\t2\t3\n", b"1\t2\t3\n") is None
    assert dc.first_difference(b"1\t2\t3\n4\t5\t6\n", b"1\t2\t3\n4\t5\t7\n").startswith("line 2: got b'4\\t5\\t6\\n'")
    assert "line 2" in dc.first_difference(b"1\t2\t3\n", b"1\t2\t3\n4\t5\t7\n")


# ---- the slice rule ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("topic_sums_slice") / "topic_sums_slice_main_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                        os.path.join(ROOT, "isle_amd", "host", "topic_sums_slice_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return out


def ask(exe, lines):
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr  # the sanitizers report on stderr
    return r.stdout.splitlines()


SLICE_PAIRS = [(0, 4), (3, 4), (4, 4), (1023, 3), (1025, 2), (2 ** 32 - 1, 4)]


def test_the_slice_rule_equals_its_restatement(exe):
    out = ask(exe, ["slice %d %d" % p for p in SLICE_PAIRS])
    for (L, W), line in zip(SLICE_PAIRS, out):
        got = [int(x) for x in line.split()]
        assert got == [dc.slice_py(L, W, q) for q in range(W + 1)], (L, W)
        lens = np.diff(got)
        assert got[0] == 0 and got[-1] == L and lens.min() >= 0 and lens.max() - lens.min() <= 1 and (np.diff(lens) <= 0).all(), (L, W)
    assert [int(x) for x in out[1].split()] == [0, 1, 2, 3, 3] and [int(x) for x in out[3].split()] == [0, 341, 682, 1023]
    assert [int(x) for x in out[4].split()] == [0, 513, 1025] and [int(x) for x in out[5].split()] == [0, 2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 32 - 1]


def test_the_gathered_form_runs_with_more_than_one_rank(exe):
    assert ask(exe, ["form %d" % w for w in (0, 1, 2, 8)]) == ["local", "local", "gathered", "gathered"]
