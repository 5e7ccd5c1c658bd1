"""CPU: the KeyFrameDatabase checker and the host parts of the detector.

  * every fixture of tests/kfdb_fixtures.py bites: tests/pyref_kfdb.py with the fixture's rule switched off
    returns other candidates, and the fixture is as small as promised;
  * the closed form of the marking that csrc/kfdb.hip computes per entry equals the restatement's walk over
    its inverted file on 300 random add / erase / re-add / clear_map / query sequences;
  * csrc/kfdb_select.h, through the library's host-only entry points and built into a stand-alone program
    with AddressSanitizer and UBSan, returns the restatement's candidates on the fixtures and on random
    sessions.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import keyframedb as K
from tests import kfdb_fixtures as FX
from tests import pyref_kfdb as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_comments_ghr_amd", "csrc")
RANDOM_SEEDS = range(300)


# ----------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("name", list(FX.BUILDERS))
def test_fixture_bites(name):
    S = FX.build(name)
    assert len(S.kfs) <= 300 and all(len(w) <= 200 and len(w) == len(v) for w, v, _ in S.kfs.values())
    if S.rule is None:
        return
    on, off = FX.bites(name)
    print(name, S.rule, "on", on, "off", off)
    assert on != off, S.doc


def test_fixture_shapes():
    """What each fixture is there for."""
    o = {k: FX.reference(k) for k in FX.BUILDERS}
    S = FX.build("connected_excluded")
    f = o["connected_excluded"][-1].fields
    assert f[1][:2] == (0, 1) and f[4][:2] == (0, 1) and f[2][0] == 60   # connected: words 1, query untouched
    assert (o["threshold_max5"][-1].max_common_words, o["threshold_max5"][-1].min_common_words) == (5, 4)
    assert (o["threshold_max1"][-1].max_common_words, o["threshold_max1"][-1].min_common_words) == (1, 0)
    assert [k for k, *_ in o["tie_identical"][-1].scored] == [10, 5, 8]
    assert [k for k, *_ in o["tie_acc_score"][-1].scored] == [2, 1]
    assert [k for k, *_ in o["tie_readd"][-1].scored] == [2, 1]
    assert o["id_zero"][-1].n_sharing == 0 and o["id_zero"][-1].fields[1][:2] == (0, 10)
    assert o["id_repeated"][-1].n_sharing == 1 and o["id_repeated"][-1].fields[1][1] == 20
    assert o["fewer_than_n"][-1].candidates == ((1,), (2,))
    assert o["bad_best"][-1].candidates[0] == (2, 3) and 1 in S.kfs
    # 0.75 exactly, against 0.75f * 1.0f
    assert [FX.bits_f32(b) for _, _, b, _ in o["reloc_strict"][-1].scored] == [1.0, 0.75]


# ----------------------------------------------------------------------------------- closed form
def closed_form(entries, qwords, qid, connected, place):
    """Steps 1 of a detector as csrc/kfdb.hip computes it: ``entries`` the KeyFrames in the database in the
    order of their (latest) add.  Updates the fields, returns the sharing list."""
    Q, W = ("mnPlaceRecognitionQuery", "mnPlaceRecognitionWords") if place else ("mnRelocQuery", "mnRelocWords")
    qs = set(qwords)
    listed = []
    for pos, k in enumerate(entries):
        common = [w for w in k.words if w in qs]
        h = len(common)
        if h == 0:
            continue
        if getattr(k, Q) != qid:
            if place and k in connected:
                setattr(k, W, 1)
            else:
                setattr(k, Q, qid)
                setattr(k, W, h)
                listed.append((common[0], pos, k))
        else:
            setattr(k, W, getattr(k, W) + h)
    return [k for _, _, k in sorted(listed, key=lambda t: (t[0], t[1]))]


@pytest.mark.parametrize("block", range(6))
def test_closed_form_equals_the_walk(block):
    for seed in RANDOM_SEEDS[block * 50:(block + 1) * 50]:
        S = FX.random_session(seed, n_kf=30, n_vocab=120, n_ops=60, max_words=25)
        a = {k: R.KeyFrame(k, w, v, m) for k, (w, v, m) in S.kfs.items()}
        b = {k: R.KeyFrame(k, w, v, m) for k, (w, v, m) in S.kfs.items()}
        db = R.KeyFrameDatabase(S.n_words)
        order = []                                   # the closed form's database: ids in add order
        for op in S.ops:
            if op[0] == "add":
                db.add(a[op[1]])
                order.append(op[1])
            elif op[0] == "erase":
                db.erase(a[op[1]])
                order.remove(op[1])
            elif op[0] == "clear_map":
                db.clear_map(op[1])
                order = [k for k in order if S.kfs[k][2] != op[1]]
            else:
                q, place = op[1], op[0] == "place"
                t = R.Trace()
                db._share_and_score(q.words, q.values, q.id, {a[c] for c in q.connected}, place, (), t)
                want_list = [k.mnId for k, *_ in t.scored]
                got = closed_form([b[k] for k in order], q.words, q.id, {b[c] for c in q.connected}, place)
                assert len(got) == t.n_sharing, (seed, op)
                W = "mnPlaceRecognitionWords" if place else "mnRelocWords"
                mx = max((getattr(k, W) for k in got), default=0)
                mn = int(np.float32(mx) * np.float32(0.8))
                assert [k.mnId for k in got if getattr(k, W) > mn] == want_list, (seed, op)
                # scores are written by the restatement only: copy them, then all six fields must agree
                for k, _, si, _ in t.scored:
                    setattr(b[k.mnId], "mPlaceRecognitionScore" if place else "mRelocScore", si)
                assert all(a[k].fields() == b[k].fields() for k in a), (seed, op)


# ----------------------------------------------------------------------------------- the selection header
def problems():
    """(session, op, outcome) of every query of the fixtures and of 40 random sessions"""
    out = []
    sessions = [FX.build(n) for n in FX.BUILDERS] + [FX.random_session(1000 + s) for s in range(40)]
    for S in sessions:
        qops = [op for op in S.ops if op[0] in ("place", "reloc")]
        for op, o in zip(qops, FX.run_ref(S)):
            out.append((S, op, o))
    return out


def test_selection_through_the_library():
    n_nonempty = 0
    for S, op, o in problems():
        cands, neighs, qid, qmap = FX.select_problem(S, op, o)
        if o.kind == "place":
            got = tuple(tuple(x) for x in K.select_nbest(cands, neighs, qid, qmap, op[2]))
        else:
            got = (tuple(K.select_reloc(cands, neighs, qid, qmap)),)
        assert got == o.candidates, (op, got, o.candidates)
        n_nonempty += any(len(c) for c in o.candidates)
    assert n_nonempty > 100


@pytest.fixture(scope="module")
def select_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("kfdb") / "kfdb_select")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(ROOT, "tests", "host", "kfdb_select.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_selection_header_clean_under_host_sanitizers(select_exe):
    def kf(t):
        return f"{t[0]} {FX.f32bits(t[1])} {t[2]} {t[3]} {t[4]} {t[5]}"
    lines, want = [], []
    for S, op, o in problems():
        cands, neighs, qid, qmap = FX.select_problem(S, op, o)
        body = " ".join(kf(c) + f" {len(nl)} " + " ".join(kf(x) for x in nl) for c, nl in zip(cands, neighs))
        if o.kind == "place":
            lines.append(f"P {len(cands)} {qid} {qmap} {op[2]} {body}")
            want.append(" ".join(["L", *map(str, o.candidates[0]), "M", *map(str, o.candidates[1])]))
        else:
            lines.append(f"R {len(cands)} {qid} {qmap} {body}")
            want.append(" ".join(["C", *map(str, o.candidates[0])]))
    r = subprocess.run([select_exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines() == want
