"""Host side of the whole program (main.cpp:36-390, crypto-recommendation_amd/
recommend.py): the printers (lshkm_tweets_coin_names, lshkm_recom_write) against
the output files the reference's own main wrote (tests/golden/main, made by
tools/gen_main_golden.cpp), the order of the program's clock readings, the
command line's refusals, and the two new host functions under ASan / UBSan in a
stand-alone program. No GPU."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import program_cases as pc
from amd import PKG, lshkm

sys.path.insert(0, PKG)
import recommend  # noqa: E402

REF = "/root/reference"
HAVE_REF = os.path.exists(os.path.join(REF, "main.cpp"))
HIPCC = "/opt/rocm/bin/hipcc"


def tweets_of(name):
    return lshkm.Tweets(pc.path(name, "tweets.csv"), pc.path(name, "lex.csv"), pc.path(name, "coins.csv"), ",", threads=1)


def test_fixtures_present_and_small():
    assert sorted(os.listdir(pc.DIR)) == sorted(pc.CASES + pc.SHARED)
    for name in pc.CASES:
        want = ["cluster.conf", "coins.csv", "expected.out", "clock.json"] + (["stdout.txt"] if name == "mid_validate" else [])
        assert sorted(os.listdir(os.path.join(pc.DIR, name))) == sorted(want)
        for f in want + ["tweets.csv", "lex.csv", "p2.csv"]:
            assert os.path.getsize(pc.path(name, f)) <= 430 * 1024, (name, f)
        conf = {ln.split(" ")[0]: ln.split(" ")[1] for ln in open(pc.path(name, "cluster.conf")).read().splitlines()}
        for key, f in (("proj_2_input", "p2.csv"), ("lexicon_file", "lex.csv"), ("query_file", "coins.csv")):
            assert os.path.normpath(os.path.join(pc.DIR, name, conf[key])) == pc.path(name, f)


@pytest.mark.parametrize("name", pc.CASES)
def test_fixture_conditions(name):
    """What the cases are there for, read off the reference's files."""
    blocks = pc.parse_blocks(pc.expected(name))
    assert [b[0] for b in blocks] == pc.TITLES
    assert [len(r) for b in blocks for r in b[2][:1]] == pc.N_TOP
    fields = pc.coin_fields(name)
    names = [f[4] if len(f) > 4 else f[0] for f in fields]
    assert len(set(names)) == len(names)                               # a printed name maps back to one index
    assert any(len(f) >= 5 for f in fields) and any(len(f) < 5 for f in fields)
    assert {n for b in blocks for row in b[2] for n in row} <= set(names)
    assert blocks[0][1] == blocks[2][1]                                # A and C list every user, in one order
    for b in blocks:
        assert [u for u in blocks[0][1] if u in set(b[1])] == b[1]
    if name == "mid_skip":
        assert 0 < len(blocks[1][1]) < len(blocks[0][1])               # block B skips users
    if name == "tiny_crlf":
        assert b"\r\n" in open(pc.path(name, "tweets.csv"), "rb").read()
        assert b"\r\n" in open(pc.path(name, "coins.csv"), "rb").read()
        assert b"\r\n" in open(pc.path(name, "p2.csv"), "rb").read()
        assert b"\r" not in pc.expected(name)
        assert len(fields) == 5                                        # fewer than 5 unknown coins: block A's rows are padded
        assert any(row[-1] == names[0] and row[-2] == names[0] for row in blocks[0][2])


@pytest.mark.parametrize("name", pc.CASES)
def test_coin_names_fall_back_to_field_0(name):
    t = tweets_of(name)
    fields = pc.coin_fields(name)
    assert t.crypto_num == len(fields)
    for idx in (4, 0, 2, 6, 1000):
        assert t.coin_names(idx) == [f[idx] if len(f) > idx else f[0] for f in fields], idx
    assert t.coin_names() == t.coin_names(4)
    with pytest.raises(lshkm.LshkmError):
        t.coin_names(-1)


@pytest.mark.parametrize("name", pc.CASES)
def test_writer_round_trip(name, tmp_path):
    """expected.out parsed into (ids, coin indexes) per block and written back:
    byte for byte the reference's file, the execution times aside. Block B goes
    through the skip flags: every user of block A, the missing ones flagged."""
    t = tweets_of(name)
    index = {n: i for i, n in enumerate(t.coin_names())}
    data = pc.expected(name)
    blocks = pc.parse_blocks(data)
    out = str(tmp_path / "out.txt")
    with open(out, "wb") as f:
        f.write(b"left over from an earlier run\n")
    everyone = blocks[0][1]
    for b, (title, ids, rows) in enumerate(blocks):
        top = {u: [index[n] for n in row] for u, row in zip(ids, rows)}
        full = np.array([top.get(u, [-1] * pc.N_TOP[b]) for u in everyone], np.int32)
        skip = np.array([u not in top for u in everyone])
        lshkm.recom_write(t, out, title, everyone, full, skip, elapsed_ms=12 + b, append=b > 0)
    got = open(out, "rb").read()
    assert pc.masked(got) == pc.masked(data)
    assert got.count(b"\r") == 0 and b"Execution Time: 13\n" in got
    # with the reference's times the bytes themselves
    for b, (title, ids, rows) in enumerate(blocks):
        lshkm.recom_write(t, out, title, ids, np.array([[index[n] for n in row] for row in rows], np.int32).reshape(
            len(ids), pc.N_TOP[b]), None, 0, append=b > 0)
    assert open(out, "rb").read() == data


def test_writer_refusals(tmp_path):
    t = tweets_of("tiny_crlf")
    out = str(tmp_path / "out.txt")
    lshkm.recom_write(t, out, "T", ["a", "b"], np.array([[0, 4], [1, 1]], np.int32), None, 3, append=False)
    before = open(out, "rb").read()
    assert before == b"T\na Bitcoin doge\nb ethereum ethereum\nExecution Time: 3\n"
    for bad in (t.crypto_num, -1, 2 ** 31 - 1):
        with pytest.raises(lshkm.LshkmError) as e:
            lshkm.recom_write(t, out, "T", ["a", "b"], np.array([[0, 4], [1, bad]], np.int32), None, 3)
        assert "lshkm error -1" in str(e.value) and "outside [0, 5)" in str(e.value)
        assert open(out, "rb").read() == before                         # checked before the file is touched
        # the same index on a skipped user is not read
        lshkm.recom_write(t, out, "T", ["a", "b"], np.array([[0, 4], [1, bad]], np.int32), [False, True], 3, append=False)
        assert open(out, "rb").read() == b"T\na Bitcoin doge\nExecution Time: 3\n"
        lshkm.recom_write(t, out, "T", ["a", "b"], np.array([[0, 4], [1, 1]], np.int32), None, 3, append=False)
    with pytest.raises(lshkm.LshkmError) as e:
        lshkm.recom_write(t, str(tmp_path / "no_such_dir" / "out.txt"), "T", ["a"], np.array([[0]], np.int32))
    assert "lshkm error -1" in str(e.value) and "no_such_dir" in str(e.value)
    with pytest.raises(lshkm.LshkmError):
        lshkm.recom_write(t, str(tmp_path), "T", ["a"], np.array([[0]], np.int32))      # a directory
    # no user, no coin: the title and the time
    lshkm.recom_write(t, out, "T", [], np.zeros((0, 5), np.int32), None, 0, append=False)
    assert open(out, "rb").read() == b"T\nExecution Time: 0\n"
    lshkm.recom_write(t, out, "T", ["", "x"], np.zeros((2, 0), np.int32), None, -1)
    assert open(out, "rb").read() == b"T\nExecution Time: 0\nT\n\nx\nExecution Time: -1\n"


@pytest.mark.parametrize("name", pc.CASES)
def test_clock_order(name):
    c = pc.clock(name)
    validate = name == "mid_validate"
    s = recommend.program_seeds(c["clock0"], validate)
    assert s["readings"] == c["readings"] == (23 if validate else 13)
    c0 = c["clock0"]
    order = ["proj2", "A_t1", "A_lsh", "A_t2"] + ["fold"] * (10 if validate else 0) + \
            ["B_t1", "B_lsh", "B_t2", "C_t1", "C_rand", "C_t2", "D_t1", "D_kpp", "D_t2"]
    got = dict((s[k], k) for k in order if k != "fold")
    got.update((v, "fold") for v in s["folds"])
    assert [got[c0 + i] for i in range(s["readings"])] == order
    if validate:
        assert s["folds"] == [c0 + i for i in range(4, 14)]               # positions 4..13
        plain = recommend.program_seeds(c0, False)
        for k in order[14:]:
            assert s[k] == plain[k] + 10                                  # every later reading moves by ten
    else:
        assert s["folds"] == []


def test_missing_flags_and_keys(tmp_path):
    with pytest.raises(lshkm.LshkmError, match="-d"):
        recommend.parse_args(["-o", "out"])
    with pytest.raises(lshkm.LshkmError, match="-o"):
        recommend.parse_args(["-d", "in", "-validate"])
    a = recommend.parse_args(["-validate", "-o", "out", "-d", "in"])
    assert (a.input, a.output, a.validate, a.config, a.clock0) == ("in", "out", True, "./cluster.conf", None)
    a = recommend.parse_args(["-d", "in", "-o", "out", "--config", "c.conf", "--clock0", "77"])
    assert (a.validate, a.config, a.clock0) == (False, "c.conf", 77)
    conf = tmp_path / "cluster.conf"
    conf.write_text("proj_2_input p2.csv\nnumber_of_hash_tables 3\n")
    with pytest.raises(lshkm.LshkmError, match="number_of_clusters"):
        recommend.run_recommendation(None, str(conf), "in", str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
    with pytest.raises(lshkm.LshkmError, match="-d"):
        recommend.run_recommendation(None, str(conf), None, "out")
    with pytest.raises(lshkm.LshkmError, match="-o"):
        recommend.run_recommendation(None, str(conf), "in", "")


def test_double_prints_as_cout_prints_it():
    assert [recommend.format_double(v) for v in (0.2781779, 1.0, 0.0, 123456789.0, 1e-7, float("inf"), 0.1 + 0.2)] == \
        ["0.278178", "1", "0", "1.23457e+08", "1e-07", "inf", "0.3"]
    assert recommend.format_double(float("nan")) == "nan" and recommend.format_double(-float("nan")) == "-nan"


@pytest.mark.skipif(not HAVE_REF, reason="reference sources absent")
def test_fixtures_reproduce(tmp_path):
    exe = tmp_path / "gen_main_golden"
    lib = os.path.join(REF, "lib")
    subprocess.run(["g++", "-std=c++11", "-O0", "-w", "-I", REF, "-I", lib, "-o", str(exe),
                    os.path.join(pc.ROOT, "tools", "gen_main_golden.cpp"), os.path.join(lib, "utils.cpp"),
                    os.path.join(lib, "data_structures", "tweet.cpp"), os.path.join(lib, "in_out", "arg_parser.cpp")],
                   check=True)
    out = tmp_path / "golden" / "main"
    out.mkdir(parents=True)
    subprocess.run([str(exe), str(out)], check=True, capture_output=True, timeout=240)
    assert sorted(os.listdir(out)) == sorted(pc.CASES + pc.SHARED)
    for sub in pc.CASES + [""]:
        files = sorted(f for f in os.listdir(os.path.join(pc.DIR, sub)) if f not in pc.CASES)
        assert sorted(f for f in os.listdir(out / sub) if f not in pc.CASES) == files
        match, mismatch, errors = filecmp.cmpfiles(os.path.join(pc.DIR, sub), out / sub, files, shallow=False)
        assert (mismatch, errors) == ([], []), sub
    # the tweet and lexicon files it shares with tests/golden/uservec: the committed ones, and it accepts them as they are
    uv = os.path.join(pc.DIR, "..", "uservec")
    made = sorted(os.listdir(tmp_path / "golden" / "uservec"))
    assert made == ["mid_lexicon.csv", "mid_tweets.csv", "tiny_lexicon.csv", "tiny_tweets.csv"]
    match, mismatch, errors = filecmp.cmpfiles(uv, tmp_path / "golden" / "uservec", made, shallow=False)
    assert (mismatch, errors) == ([], [])
    (tmp_path / "golden" / "uservec" / "tiny_tweets.csv").write_bytes(b"P,3\n")
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "tiny_tweets.csv differs" in r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_printers_under_asan_ubsan(tmp_path):
    """lshkm_tweets_coin_names and lshkm_recom_write in a stand-alone host program
    (tests/program_asan.cpp) built with -fsanitize=address,undefined on the host
    side only, over the tiny case. CPU only; nothing is loaded into Python."""
    exe = str(tmp_path / "program_asan")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
           "-I" + os.path.join(pc.ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
           os.path.join(pc.ROOT, "tests", "program_asan.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    work = tmp_path / "work"
    work.mkdir()
    tiny = [pc.path("tiny_crlf", f) for f in ("tweets.csv", "lex.csv", "coins.csv", "expected.out")]
    r = subprocess.run([exe, str(work)] + tiny, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "program_asan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
