"""The whole-program fixtures (tests/golden/main, written by
tools/gen_main_golden.cpp from the reference's own main) and the helpers the
CPU and the GPU test of the program share."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "main")
CASES = ["mid", "mid_skip", "mid_validate", "tiny_crlf"]
SHARED = ["mid_p2.csv", "tiny_p2.csv"]                   # the project-2 vectors; tweets and lexicon: tests/golden/uservec
TIME = "Execution Time: "
TITLES = ["Cosine LSH", "Cosine LSH", "Clustering Recommendation", "Clustering Recommendation"]
N_TOP = [5, 2, 5, 2]


def kind(name):
    return "tiny" if name.startswith("tiny") else "mid"


def path(name, file):
    """A file of case `name`; tweets.csv, lex.csv and p2.csv are the shared files
    its cluster.conf points at."""
    shared = {"tweets.csv": os.path.join(DIR, "..", "uservec", kind(name) + "_tweets.csv"),
              "lex.csv": os.path.join(DIR, "..", "uservec", kind(name) + "_lexicon.csv"),
              "p2.csv": os.path.join(DIR, kind(name) + "_p2.csv")}
    return os.path.normpath(shared[file]) if file in shared else os.path.join(DIR, name, file)


def clock(name):
    with open(path(name, "clock.json")) as f:
        return json.load(f)


def expected(name):
    with open(path(name, "expected.out"), "rb") as f:
        return f.read()


def masked(data):
    """The file's lines with the execution times masked."""
    lines = data.split(b"\n")
    return [TIME.encode() if ln.startswith(TIME.encode()) else ln for ln in lines]


def parse_blocks(data):
    """[(title, [user id], [[coin name]])] of an output file."""
    text = data.decode()
    assert text.endswith("\n")
    blocks, cur = [], None
    for ln in text[:-1].split("\n"):
        if cur is None:
            cur = (ln, [], [])
        elif ln.startswith(TIME):
            blocks.append(cur)
            cur = None
        else:
            f = ln.split(" ")
            cur[1].append(f[0])
            cur[2].append(f[1:])
    assert cur is None
    return blocks


def coin_fields(name):
    """The coin file's lines as file_to_str_vectors splits them."""
    with open(path(name, "coins.csv"), "rb") as f:
        lines = f.read().decode().split("\n")[:-1]
    return [ln[:-1].split(",") if ln.endswith("\r") else ln.split(",") for ln in lines]
