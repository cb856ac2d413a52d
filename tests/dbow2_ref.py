"""oracle/_ref/dbow2_ref: the reference's own Thirdparty/DBoW2 behind a command line (oracle/dbow2_ref_driver.cpp, built by
`make -C oracle ref` where the reference checkout exists; the binary travels to machines without one).  Everything here feeds it
bytes and parses what it prints; nothing reads the reference tree."""
import os
import subprocess

import numpy as np

import vocab_synth as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "dbow2_ref")

# (k, L, levelsup): the 16 | 17 pair are the two sides of the kernel's lane-group switch, (2, 10) the deepest tree the text
# format allows, levelsup >= L puts every feature into node 0
SHAPES = [(10, 4, 2), (3, 5, 4), (7, 4, 0), (10, 3, 1), (16, 3, 1), (17, 3, 2), (20, 3, 0), (2, 10, 5), (10, 3, 4), (10, 3, 7)]
PAIRS = [(scoring, weighting) for scoring in range(6) for weighting in range(4)]


_made = []


def require():
    if not _made:  # as oracle_py builds its library on demand: brings the binary up to date where the reference checkout exists,
        _made.append(subprocess.call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"]))  # does nothing where it does not
        assert _made[0] == 0, "make -C oracle ref failed with the reference checkout present"
    assert os.path.isfile(BIN) and os.access(BIN, os.X_OK), (
        "%s is missing: build() makes it where the reference checkout exists (make -C oracle ref) and it has to travel with the "
        "tree to a machine that has none -- there is no skip path, the vocabulary path is pinned by this binary" % BIN)
    return BIN


def run(*args):
    return subprocess.run([require()] + [str(a) for a in args], check=True, stdout=subprocess.PIPE).stdout.decode()


def tree(k, L, seed, early_leaf_p=0.0, dup_p=0.4, stop_p=0.3, children=None):
    return vs.make_tree(k, L, seed=seed, early_leaf_p=early_leaf_p, dup_p=dup_p, stop_p=stop_p, children=children)


def tree_root65(seed=1, dup_p=0.4, stop_p=0.3):
    """65 children under the root (one more than a 64-lane group holds), 3 below, under a header that says k = 20: the header's
    k only sizes a reserve() in the reference's loader"""
    return tree(20, 3, seed, dup_p=dup_p, stop_p=stop_p, children=lambda pid, d: 65 if d == 0 else 3)


def tree_one17(seed=4, dup_p=0.4, stop_p=0.3):
    """3 children everywhere except node 1 (the root's first child), which has 17: maxChildren alone is above 16"""
    return tree(17, 4, seed, dup_p=dup_p, stop_p=stop_p, children=lambda pid, d: 17 if pid == 1 else 3)


def widest_last_child(t):
    """the last child of the (first) node with the most children"""
    pid = int(np.argmax(np.diff(t["childOff"])))
    return int(t["childIdx"][t["childOff"][pid + 1] - 1])


def text(t, scoring=0, weighting=0, final_newline=False):
    """the text vocabulary of vocab_synth.write_text; by default WITHOUT the newline behind the last node, because the
    reference's `while(!f.eof())` loop makes one more node out of it"""
    if "_body" not in t:  # the node lines, made once per tree
        lines = []
        for i in range(1, len(t["parent"])):
            leaf = t["childOff"][i + 1] == t["childOff"][i]
            lines.append("%d %d %s %r" % (t["parent"][i], 1 if leaf else 0, " ".join(str(int(v)) for v in t["nodeDesc"][i]), float(t["weight"][i])))
        t["_body"] = "\n".join(lines)
    return "%d %d %d %d\n" % (t["k"], t["L"], scoring, weighting) + t["_body"] + ("\n" if final_newline else "")


def parse_transform(out):
    lines = out.split("\n")
    nb, nf, nw = (int(x) for x in lines[0].split())
    bow = [(int(l.split()[0]), float.fromhex(l.split()[1])) for l in lines[1:1 + nb]]
    fv = {}
    for l in lines[1 + nb:1 + nb + nf]:
        x = [int(v) for v in l.split()]
        assert x[1] == len(x) - 2
        fv[x[0]] = x[2:]
    assert len(bow) == nb and len(fv) == nf
    return nw, bow, fv


def transform(tmp, voc_text, desc, levelsup):
    """-> (nWords, BowVector as ordered [(word, double)], FeatureVector as {node: [feature...]} in the printed (ascending) order)"""
    voc, d = os.path.join(str(tmp), "ref_voc.txt"), os.path.join(str(tmp), "ref_desc.bin")
    with open(voc, "w") as f:
        f.write(voc_text)
    np.ascontiguousarray(desc, np.uint8).tofile(d)
    return parse_transform(run("transform", voc, d, levelsup))


def resave(tmp, voc_text):
    src, dst = os.path.join(str(tmp), "ref_in.txt"), os.path.join(str(tmp), "ref_out.txt")
    with open(src, "w") as f:
        f.write(voc_text)
    run("resave", src, dst)
    return dst


def distance(tmp, a, b):
    p = os.path.join(str(tmp), "ref_pairs.bin")
    np.concatenate([np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)], axis=1).tofile(p)
    return np.array([int(x) for x in run("distance", p).split()], np.int64)


def randomint(seed, ds):
    return [int(x) for x in run("randomint", seed, *ds).split()]


def ours(t, desc, levelsup, scoring, weighting, triples=None):
    """the same three things from this project's C oracle (the descent; `triples` = an earlier call's) + test_vocab.ref_bow
    (the assembly)"""
    import oracle_py as O
    from test_vocab import ref_bow
    if triples is None:
        triples = O.vocab_transform(t["childOff"], t["childIdx"], t["nodeDesc"], t["wordId"], t["weight"], t["L"], desc, levelsup)
    bow, fv = ref_bow(triples[0], triples[1], triples[2], weighting, scoring)
    return t["nWords"], list(bow.items()), fv, triples


def node_of(fv, n):
    """FeatureVector -> the node of every feature, -1 where it is in none"""
    node = np.full(n, -1, np.int64)
    for g, idx in fv.items():
        assert (node[idx] == -1).all() and idx == sorted(idx)
        node[idx] = g
    return node
