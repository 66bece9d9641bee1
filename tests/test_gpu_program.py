"""GPU parity: the whole program (crypto-recommendation_amd/recommend.py,
main.cpp:36-390) against the output files the reference's own main wrote for
the same inputs and the same clock (tests/golden/main, made by
tools/gen_main_golden.cpp): the four blocks line for line, the skipped users,
the 10-fold value the program prints, and the ten-reading shift of every later
seed under -validate. Each case runs once; the tests share the run."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import program_cases as pc
from amd import PKG, lshkm

sys.path.insert(0, PKG)
import recommend  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def run_case(ctx, name, out):
    c = pc.clock(name)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        res = recommend.run_recommendation(ctx, pc.path(name, "cluster.conf"), pc.path(name, "tweets.csv"), str(out),
                                           validate=name == "mid_validate", clock0=c["clock0"], time0=c["time0"])
    with open(out, "rb") as f:
        return res, f.read(), printed.getvalue()


@pytest.fixture(scope="module")
def runs(ctx, tmp_path_factory):
    """name -> (returned dict, the output file's bytes, what was printed), each case run once."""
    done = {}
    tmp = tmp_path_factory.mktemp("program")

    def get(name):
        if name not in done:
            done[name] = run_case(ctx, name, tmp / (name + ".out"))
        return done[name]
    return get


def names_of(name):
    fields = pc.coin_fields(name)
    return np.array([f[4] if len(f) > 4 else f[0] for f in fields], dtype=object)


@pytest.mark.parametrize("name", pc.CASES)
def test_output_file_is_the_references(runs, name):
    res, data, _ = runs(name)
    want = pc.expected(name)
    got_lines, want_lines = pc.masked(data), pc.masked(want)
    bad = [i for i, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b]
    assert not bad and len(got_lines) == len(want_lines), (len(got_lines), len(want_lines), bad[:5],
                                                           [(got_lines[i], want_lines[i]) for i in bad[:3]])
    # the returned arrays say what the file says
    names = names_of(name)
    blocks = pc.parse_blocks(want)
    for b, blk in enumerate("ABCD"):
        r = res["blocks"][blk]
        assert r["top"].shape == (len(res["user_ids"]), pc.N_TOP[b]) and r["top"].dtype == np.int32
        assert r["skip"].dtype == bool and list(r["ids"]) == list(res["user_ids"])
        keep = ~r["skip"]
        assert list(r["ids"][keep]) == blocks[b][1], blk
        assert [list(row) for row in names[r["top"][keep]]] == blocks[b][2], blk
    assert not res["blocks"]["A"]["skip"].any() and not res["blocks"]["C"]["skip"].any()
    assert list(res["users"]["ids"]) == list(res["user_ids"]) == blocks[0][1]
    assert res["users"]["x"].shape == (len(blocks[0][1]), len(names)) and res["users"]["x"].dtype == np.float64
    assert res["fake_users"]["x"].shape[1] == len(names) and res["fake_users"]["x"].shape[0] >= 1
    assert res["seeds"] == recommend.program_seeds(pc.clock(name)["clock0"], name == "mid_validate")
    assert (res["validation"] is None) == (name != "mid_validate")


def test_block_b_skips_exactly_the_missing_users(runs):
    res, _, _ = runs("mid_skip")
    blocks = pc.parse_blocks(pc.expected("mid_skip"))
    skip = res["blocks"]["B"]["skip"]
    missing = set(blocks[0][1]) - set(blocks[1][1])
    assert missing and set(res["user_ids"][skip]) == missing
    assert 0 < skip.sum() < len(skip)


def test_validate_prints_the_references_value(runs):
    res, _, printed = runs("mid_validate")
    with open(pc.path("mid_validate", "stdout.txt")) as f:
        want = [ln for ln in f.read().split("\n") if ln.startswith(" aa")]
    got = [ln for ln in printed.split("\n") if ln.startswith(" aa")]
    assert len(want) == 1 and got == want
    assert got[0] == " aa" + recommend.format_double(res["validation"])


def test_validate_moves_every_later_seed_by_ten(runs):
    # the file of the -validate run equals its own expected.out: blocks B, C and
    # D were seeded by readings 15, 18 and 21, not 5, 8 and 11
    res, data, _ = runs("mid_validate")
    c0 = pc.clock("mid_validate")["clock0"]
    assert (res["seeds"]["B_lsh"], res["seeds"]["C_rand"], res["seeds"]["D_kpp"]) == (c0 + 15, c0 + 18, c0 + 21)
    assert res["seeds"]["folds"] == list(range(c0 + 4, c0 + 14))
    assert pc.masked(data) == pc.masked(pc.expected("mid_validate"))


def test_duplicated_project2_ids_are_refused(ctx, tmp_path):
    # the reference's k_means_pp keys its distance cache by row ID
    # (initialization.hpp:97-109): rows sharing an ID share distances there
    with open(pc.path("tiny_crlf", "p2.csv"), "rb") as f:
        rows = f.read()
    (tmp_path / "p2.csv").write_bytes(rows + rows.split(b"\r\n")[0].replace(b"0.", b"1.") + b"\r\n")
    conf = open(pc.path("tiny_crlf", "cluster.conf")).read()
    for key, f in (("proj_2_input", str(tmp_path / "p2.csv")), ("lexicon_file", pc.path("tiny_crlf", "lex.csv")),
                   ("query_file", pc.path("tiny_crlf", "coins.csv"))):
        conf = "\n".join(key + " " + f if ln.startswith(key + " ") else ln for ln in conf.split("\n"))
    (tmp_path / "cluster.conf").write_text(conf)
    with pytest.raises(lshkm.LshkmError, match="duplicated row IDs"):
        recommend.run_recommendation(ctx, str(tmp_path / "cluster.conf"), pc.path("tiny_crlf", "tweets.csv"),
                                     str(tmp_path / "out"), clock0=1, time0=1)
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("name", ["tiny_crlf", "mid_skip"])
def test_second_call_on_the_same_context(ctx, runs, name, tmp_path):
    _, first, _ = runs(name)
    res, again, _ = run_case(ctx, name, tmp_path / "again.out")
    assert pc.masked(again) == pc.masked(first)
    assert os.path.getsize(tmp_path / "again.out") == len(again)
