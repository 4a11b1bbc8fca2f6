"""Exchange kernels on a REUSED workspace: the case table of tests/test_gpu_workspace_reuse.py, the tag check it applies to the
workspace bytes around every launch, and what can be checked without a GPU.

The protocol (csrc/xch_common.h:4-16): a caller-owned workspace is zero-filled once; every launch reads an epoch base from the
header, writes only tags in (base, base + span] and leaves base + span for the next launch; a stale granule of any earlier launch
therefore never carries the tag a later launch waits for.  A test that repeats a call with the SAME data cannot see a launch that
consumed a stale granule - it would read the value it was going to get anyway - so the GPU module runs other data, other shapes
and other kernels on one workspace and compares with a fresh one, and reads the tags themselves.

ROWS          one row per exchanging launch: the forms of tests/test_guarded_views_host.py (trace name, knobs, F of the form's
              own row) without the `generic` and `stepped` ones, which exchange nothing, plus the two-launch cluster decode and
              the two-layer BPTT at width 512.  `sites`: the xch_account( call sites the row reaches, as (file, ordinal in file).
tag_report    the violations of the tag invariant between two snapshots of [256, 256 + kXchBytes).
IDENTITY      per kind of row, which outputs are per-sequence and which are sums over the batch, where the order of such a sum was
              read, and so which outputs must be the same bits whatever the number of groups.
ROUNDS        the launchers that take min(tiles, max_groups) groups, their workgroups per group G, and per row the two resident
              limits G (one group, three rounds at B = 33) and 2 G (two groups, a ragged last round) - or the reason a pair is left out."""
import os
import re

import numpy as np
import pytest

import test_guarded_views_host as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "longterm360fov_amd", "csrc")

# csrc/xch_common.h
ST_TIMEOUT, ST_LAUNCHES, ST_EPOCH = 0, 2, 3
STATUS_BYTES = 256
XCH_BYTES = 64 << 20
ARRIVE_WORDS, ARRIVE_STRIDE = 64, 32            # 64 arrival words 128 bytes apart, the last 8 KB of the area
REZERO_ABOVE = 0x70000000                       # xch_account (api_state.hip) re-zeroes header and granules beyond this
EPOCH_BASES = (1, 2, 0x6F000000, REZERO_ABOVE - 5)

# the shapes of check A (and C, E: the first); D: B = 33
SHAPES = ((30, 3), (17, 2), (30, 3))
ROUNDS_B = 33


# ---------------------------------------------------------------------------------------------------------------------
# the tag invariant
# ---------------------------------------------------------------------------------------------------------------------
def tag_report(before, after, base0, base1, arrive_words=ARRIVE_WORDS, arrive_stride=ARRIVE_STRIDE):
    """before, after: the 32-bit words of the granule area [256, 256 + kXchBytes) in front of and behind a launch (uint32; the
    tags are the odd words: every granule and hello word is eight bytes, the tag its upper half).  base0, base1: ST_EPOCH in
    front of and behind it.  -> a list of violations, empty when
        every tag <= base1, every tag that changed lies in (base0, base1], no tag has its top bit set, and
        the arrival words (the last arrive_words * arrive_stride words of the area, one every arrive_stride) are 0 again."""
    before, after = np.asarray(before, np.uint32), np.asarray(after, np.uint32)
    assert before.shape == after.shape and before.ndim == 1 and before.size % 2 == 0 and before.size >= arrive_words * arrive_stride
    b, a = before[1::2], after[1::2]
    out = []

    def some(what, mask):
        idx = np.flatnonzero(mask)
        if idx.size:
            out.append("%s: %d tags, first at word %d (tag 0x%08x, was 0x%08x; base 0x%08x -> 0x%08x)" % (
                what, idx.size, 2 * int(idx[0]) + 1, int(a[idx[0]]), int(b[idx[0]]), base0, base1))
    some("a tag above the new base", a > np.uint32(base1))
    changed = a != b
    some("a changed tag outside (base0, base1]", changed & ((a <= np.uint32(base0)) | (a > np.uint32(base1))))
    some("a tag with its top bit set", (a >> np.uint32(31)) != 0)
    arrive = after[after.size - arrive_words * arrive_stride::arrive_stride]
    left = np.flatnonzero(arrive)
    if left.size:
        out.append("arrival word %d left at %d (%d words are not 0)" % (int(left[0]), int(arrive[left[0]]), left.size))
    return out


def _synthetic(base0=40, base1=47):
    rng = np.random.default_rng(7)
    n = 4096 + ARRIVE_WORDS * ARRIVE_STRIDE
    before = np.zeros(n, np.uint32)
    before[0:2048:2] = rng.integers(0, 1 << 32, 1024, dtype=np.uint32)        # values: any bits
    before[1:2048:2] = rng.integers(0, base0 + 1, 1024, dtype=np.uint32)      # stale tags of earlier launches
    after = before.copy()
    after[0:1024:2] = rng.integers(0, 1 << 32, 512, dtype=np.uint32)
    after[1:1024:2] = rng.integers(base0 + 1, base1 + 1, 512, dtype=np.uint32)
    return before, after, base0, base1


def test_tag_report_passes_a_clean_launch():
    assert tag_report(*_synthetic()) == []
    before, after, b0, b1 = _synthetic()
    assert tag_report(before, before, b0, b0) == []         # a launch that exchanged nothing


@pytest.mark.parametrize("mistake,says", [("above", "above the new base"), ("stale", "outside"), ("arrival", "arrival word"), ("top", "top bit")])
def test_tag_report_sees_each_mistake(mistake, says):
    before, after, b0, b1 = _synthetic()
    if mistake == "above":
        after[101] = b1 + 1                                  # one epoch past what the launch declared
    elif mistake == "stale":
        after[101] = b0 if before[101] != b0 else b0 - 1     # a granule rewritten with a tag an earlier launch could have used
        assert after[101] != before[101]
    elif mistake == "top":
        after[101] = 0x80000001
    else:
        after[after.size - ARRIVE_WORDS * ARRIVE_STRIDE + 5 * ARRIVE_STRIDE] = 1
    report = tag_report(before, after, b0, b1)
    assert report and any(says in line for line in report), report
    if mistake == "stale":
        after[101] = b0                                      # exactly base0, changed or not
        before[101] = b0 - 1
        assert any("outside" in line for line in tag_report(before, after, b0, b1))


# ---------------------------------------------------------------------------------------------------------------------
# which outputs must be the same bits whatever the number of groups (check D compares runs with 1, 2 and 3 groups)
# ---------------------------------------------------------------------------------------------------------------------
# kind -> (outputs that are per-sequence or summed in an order that does not depend on the group count: bit-identical;
#          outputs formed behind the recurrence by products whose split the launcher derives from the CU count: fp64 bound;
#          where it was read)
IDENTITY = {
    "layer": (("hs", "hT", "cT", "res"), (), "per sequence: a tile's rows are walked by one group whatever the group count"),
    "zx": (("hs", "hT", "cT", "res"), (), "per sequence"),
    "decode": (("out", "hT", "cT"), (), "per sequence; the Dense head's partials are summed per tile in slice order (lstm_cluster.hip MODE_DECODE)"),
    "decoder": (("out",), (), "per sequence"),
    "stack2": (("hs1", "hT1", "cT1", "res1", "hs2", "hT2", "cT2", "res2"), (), "per sequence; one tile per group by its shape test"),
    # db: the kernels write per-TILE partials db_part[tile] (lstm_bwd_cluster.hip:300, lstm_bwd8.hip:278 / :517, lstm_bwd16.hip:458), summed
    # by colsum, whose chunks depend on the row count alone (reduce_defer.hip:301): the order does not depend on the group count.
    # dK, dR (and dx where the kernel does not form it) are products behind the recurrence; gemm_f32 derives its split from the CU
    # count (gemm_f32.hip:361), which FOV_DBG_RESIDENT_LIMIT changes: compared with fp64 at check_grads in D, bit-identical in A, C, E.
    "backward": (("dz", "dh0", "dc0", "db"), ("dK", "dR", "dx"), "db from per-tile partials; dK, dR, dx by products"),
    "stack2_bwd": (("dz1", "dz2", "dh0_1", "dc0_1", "dh0_2", "dc0_2", "db1", "db2"), ("dK1", "dR1", "dK2", "dR2"), "as backward; not in D (one tile per group)"),
    "mix_fwd": (("M", "P", "H1", "C1", "H2", "C2", "res1", "res2"), (), "per sequence"),
    # the fused decoder's backward writes gate gradients per step and sequence; its weight gradients are products the caller forms
    "mix_bwd": (("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0"), (), "per sequence: no sum over the batch in the kernel"),
}

# launcher -> (file, workgroups per group as a function of H): the launchers that take min(num_tiles, max_groups) groups
ROUNDS = {
    "cluster layer": ("lstm_cluster.hip", lambda H: H // 64),
    "cluster decoder": ("lstm_cluster.hip", lambda H: H // 64),
    "two-launch decode": ("lstm_cluster.hip", lambda H: H // 64),
    "lstm_wide": ("lstm_wide.hip", lambda H: 16 if H == 512 else 8),
    "wide16 layer": ("lstm_wide16.hip", lambda H: H // 16),
    "lstm_layer_bf16": ("lstm_layer_bf16.hip", lambda H: 8),
    "lstm_s2s_bf16": ("lstm_s2s_bf16.hip", lambda H: 8),
    "lstm_bwd_cluster": ("lstm_bwd_cluster.hip", lambda H: H // 64),
    "lstm_bwd8": ("lstm_bwd8.hip", lambda H: 8),
    "lstm_bwd16": ("lstm_bwd16.hip", lambda H: 16),
    "mix_decoder": ("mix_decoder.hip", lambda H: 8),
    "mix_decoder_bf16": ("mix_decoder_bf16.hip", lambda H: 8),
    "mix_decoder_bwd": ("mix_decoder_bwd.hip", lambda H: 8),
    "mix_decoder_bwd_bf16": ("mix_decoder_bwd_bf16.hip", lambda H: 8),
}
# a launcher of the list above whose round loop no entry point reaches: every (form, limit) pair of it is left out
UNREACHABLE_ROUNDS = {
    "wide16 layer": "wide16_shape (lstm_wide16.hip:1067) admits the form only while tiles <= CUs / (H / 16): under a limit of G or 2 G "
                    "CUs three tiles go to another kernel, and the form has no explicit impl",
}
W16_DROPPED = "tiles <= CUs / (H / 16) is part of the form's shape test: three tiles on one or two groups go to another kernel"


def _row(name, kind, form, launched, H, F, sites, knobs=None, impl=None, dtype="f32", rounds=None, dropped=None, extra=None):
    """rounds: the launcher of ROUNDS the row belongs to (None: not in D); dropped: {1 or 2: reason} - limits (in units of G) left out.
    settles: how many of the row's launches read and rewrite the header.  All of them - except at width 64 on the cluster kernels,
    where a group is ONE workgroup: the launch passes its xch_account site on the host but touches neither header nor granules
    (G > 1 in front of every xch_ call: lstm_cluster.hip:560 `xch_used`, lstm_bwd_cluster.hip:80 / :315).  Such a row must leave
    ST_EPOCH, ST_LAUNCHES and the whole granule area as they were."""
    settles = 0 if H == 64 and set(launched) <= {"cluster", "fused cluster", "bwd cluster"} else len(launched)
    return dict(name=name, kind=kind, form=form, launched=list(launched), H=H, F=F, sites=list(sites), knobs=dict(knobs or {}), impl=impl,
                dtype=dtype, rounds=rounds, dropped=dict(dropped or {}), settles=settles, **(extra or {}))


def _rows():
    rows = []
    B30 = G.BATCHES.index(30)                     # F: the form's own row at B = 30
    for f in G.LAYER_FORMS:
        name, launched, dtype, impl, H, knobs, shapes = f
        if launched == "generic":
            continue
        F = shapes[B30][0]
        if launched == "cluster":
            site, rounds, dropped = ("lstm_cluster.hip", 0), "cluster layer", None
        elif launched == "wide LSTM":
            site, rounds, dropped = ("lstm_wide.hip", 0), "lstm_wide", None
        elif launched == "wide16 LSTM":
            site, rounds, dropped = ("lstm_wide16.hip", 0), "wide16 layer", {1: W16_DROPPED, 2: W16_DROPPED}
        else:
            site, rounds, dropped = ("lstm_layer_bf16.hip", 0), "lstm_layer_bf16", None
        rows.append(_row(name, "layer", f, [launched], H, F, [site], knobs, impl, dtype, rounds, dropped))
    for f in G.BACKWARD_FORMS:
        name, launched, dtype, H, knobs, shapes = f
        if launched == "lstm_bwd_pointwise":
            continue
        F = shapes[B30][0]
        dropped = None
        if launched == "bwd cluster":
            site, rounds = ("lstm_bwd_cluster.hip", 0), "lstm_bwd_cluster"
        elif launched == "8-group BPTT":
            site, rounds = ("lstm_bwd8.hip", 0), "lstm_bwd8"
        else:
            site, rounds = ("lstm_bwd16.hip", 0), "lstm_bwd16"
            if H != 512:
                why = "bwd16_takes (lstm_bwd16.hip:507) admits widths 128 / 256 only while tiles <= CUs / (H / 16): lstm_seq_bwd has no explicit form"
                dropped = {1: why, 2: why}
            elif knobs.get("FOV_BWD16_GROUPS") == "32":
                why = "the 32-workgroup form needs tiles <= CUs / 32 (lstm_bwd16.hip:546): under either limit the 16-workgroup form of bwd16-512 runs"
                dropped = {1: why, 2: why}
        # FOV_NO_WGRAD_GROUP=1: db is then the sum the BPTT kernel formed over its own rows (the per-tile partials of IDENTITY)
        rows.append(_row(name, "backward", f, [launched], H, F, [site], dict(knobs, FOV_NO_WGRAD_GROUP="1"), None, dtype, rounds, dropped))
    for f in G.DECODE_FORMS:
        name, launched, dtype, impl, H, shapes = f
        if launched == "generic":
            continue
        F = shapes[B30][0]
        if launched == "fused cluster":
            site, rounds = ("lstm_cluster.hip", 1), None        # one tile per group is its gate (lstm_cluster.hip:1552): no rounds by construction
        elif launched == "seq2seq decode (wide16)":
            site, rounds = ("lstm_wide16.hip", 2), None         # num_groups = num_tiles
        else:
            site, rounds = ("lstm_s2s_bf16.hip", 0), "lstm_s2s_bf16"
        rows.append(_row(name, "decode", f, [launched], H, F, [site], None, impl, dtype, rounds))
    rows.append(_row("decode-two-launches-256", "decode", None, ["cluster", "cluster"], 256, 96, [("lstm_cluster.hip", 2)], {"FOV_TWO_LAUNCHES": "1"},
                     "cluster", "f32", "two-launch decode"))
    for f in G.DECODER_FORMS:
        name, launched, impl, H, _ = f
        if launched == "generic":
            continue
        site, rounds = (("lstm_cluster.hip", 3), "cluster decoder") if launched == "cluster" else (("lstm_wide16.hip", 2), None)
        rows.append(_row(name, "decoder", f, [launched], H, G.F_DEC, [site], None, impl, "f32", rounds))
    for f in G.ZX_FORMS:
        name, launched, impl, H, _ = f
        if launched == "generic":
            continue
        site, rounds = (("lstm_cluster.hip", 0), "cluster layer") if launched == "cluster" else (("lstm_wide.hip", 0), "lstm_wide")
        rows.append(_row(name, "zx", f, [launched], H, 90, [site], None, impl, "f32", rounds))
    for f in G.STACK2_FORMS:
        name, launched, dtype, H, shapes = f
        site = ("lstm_wide16.hip", 1) if dtype == "f32" else ("lstm_stack2_bf16.hip", 0)
        rows.append(_row(name, "stack2", f, [launched], H, shapes[B30][0], [site], None, None, dtype))
    # the two-layer BPTT of the guarded tables is fov_lstm_stack2_bwd at width 512, lstm_bwd16.hip's second site: one row
    rows.append(_row("stack2-bwd-512", "stack2_bwd", G.STACK2_FORMS[0], ["two-layer BPTT"], 512, G.STACK2_FORMS[0][4][B30][0], [("lstm_bwd16.hip", 1)],
                     {"FOV_NO_WGRAD_GROUP": "1"}))
    for f in G.MIX_FORMS:
        name, dtype, _ = f
        sfx = "_bf16" if dtype == "bf16" else ""
        rows.append(_row(name, "mix_fwd", f, ["mix_decoder" + sfx], G.MIX_H, G.MIX_O, [("mix_decoder%s.hip" % sfx, 0)], None, None, dtype, "mix_decoder" + sfx))
        rows.append(_row(name + "-bwd", "mix_bwd", f, ["mix_decoder_bwd" + sfx], G.MIX_H, G.MIX_O, [("mix_decoder_bwd%s.hip" % sfx, 0)], None, None, dtype,
                         "mix_decoder_bwd" + sfx))
    return rows


ROWS = _rows()
ROW_IDS = [r["name"] for r in ROWS]


def identity(row):
    """(bit-identical outputs, outputs held to the fp64 bound) of one row in check D: IDENTITY of its kind, with dx moved to the
    bit-identical set where the eight-workgroup kernel forms it itself - 256 -> 256 with aligned K and dx (plan_lstm_bwd,
    lstm_train.hip): fp32 as eight partial tapes, one per workgroup of the group, reduced in slice order (`dx_parts`, splitk_reduce
    over 8); bf16 from the dz tile a group has gathered, per sequence.  Neither order depends on the group count."""
    bits, bound, _ = IDENTITY[row["kind"]]
    if row["kind"] == "backward" and row["launched"] == ["8-group BPTT"] and row["F"] == 256:
        bits, bound = bits + ("dx",), tuple(k for k in bound if k != "dx")
    return bits, bound


def rounds_cases(rows=None):
    """(row, limit in CUs, groups) for every (form, limit) pair of check D that is kept."""
    out = []
    for r in (ROWS if rows is None else rows):
        if r["rounds"] is None:
            continue
        g = ROUNDS[r["rounds"]][1](r["H"])
        out += [(r, k * g, k) for k in (1, 2) if k not in r["dropped"]]
    return out


def dropped_pairs():
    return [(r["name"], k, r["dropped"][k]) for r in ROWS for k in sorted(r["dropped"])]


# ---------------------------------------------------------------------------------------------------------------------
# the table against the sources
# ---------------------------------------------------------------------------------------------------------------------
def account_sites():
    """(file, ordinal) of every call of xch_account( in csrc/*.hip (its definition in api_state.hip is none)."""
    sites = []
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith(".hip"):
            continue
        with open(os.path.join(CSRC, fn)) as f:
            calls = [l for l in f if re.search(r"\bxch_account\(", l) and not re.match(r"\s*(int|void)\s+xch_account\(", l)]
        sites += [(fn, i) for i in range(len(calls))]
    return sites


def uncovered_sites(rows):
    have = {tuple(s) for r in rows for s in r["sites"]}
    return [s for s in account_sites() if s not in have]


def test_every_exchange_launch_site_has_a_row():
    sites = account_sites()
    assert len(sites) == 19 and len({f for f, _ in sites}) == 13, sites      # a new launcher moves these numbers: give it a row
    assert uncovered_sites(ROWS) == []
    assert {tuple(s) for r in ROWS for s in r["sites"]} <= set(sites), "a row names a site that is not there"


def test_the_coverage_test_fails_when_a_row_is_removed():
    for victim in ("decode-two-launches-256", "stack2-bwd-512", "mix-decoder-bf16-bwd", "stack2-bf16"):
        rest = [r for r in ROWS if r["name"] != victim]
        assert len(rest) == len(ROWS) - 1 and uncovered_sites(rest), victim


def test_rows_are_the_guarded_forms_without_the_ones_that_exchange_nothing():
    names = {r["name"] for r in ROWS}
    assert len(names) == len(ROWS)
    for table, launched_at in ((G.LAYER_FORMS, 1), (G.BACKWARD_FORMS, 1), (G.DECODE_FORMS, 1), (G.DECODER_FORMS, 1), (G.ZX_FORMS, 1), (G.STACK2_FORMS, 1)):
        for f in table:
            assert (f[0] in names) == (f[launched_at] not in ("generic", "lstm_bwd_pointwise")), f[0]
    assert {f[0] for f in G.MIX_FORMS} | {f[0] + "-bwd" for f in G.MIX_FORMS} <= names
    assert sorted(r["name"] for r in ROWS if r["settles"] == 0) == ["bwd_cluster-64", "cluster-64", "decode-cluster-64", "decoder-cluster-64"]
    for fn, needle in (("lstm_cluster.hip", "const bool xch_used = (G > 1) &&"), ("lstm_bwd_cluster.hip", "if (G > 1) xch_settle(")):
        with open(os.path.join(CSRC, fn)) as f:
            assert needle in f.read(), (fn, needle)
    for r in ROWS:
        assert all(T <= 3 and B <= 33 for B, T in SHAPES) and r["kind"] in IDENTITY and r["launched"], r["name"]
        if r["form"] is not None and r["kind"] in ("layer", "backward", "decode", "stack2"):
            shapes = r["form"][{"layer": 6, "backward": 5, "decode": 5, "stack2": 4}[r["kind"]]]
            assert r["F"] in {s[0] for s in shapes}, r["name"]


def test_identity_rule_names_every_output_once():
    in_kernel_dx = sorted(r["name"] for r in ROWS if "dx" in identity(r)[0])
    assert in_kernel_dx == ["bwd8-256", "bwd8-256-bf16"], in_kernel_dx
    assert all(set(identity(r)[0]) | set(identity(r)[1]) == set(IDENTITY[r["kind"]][0]) | set(IDENTITY[r["kind"]][1]) for r in ROWS)
    for kind, (bits, bound, where) in IDENTITY.items():
        assert bits and not set(bits) & set(bound) and where, kind
    # the sources still say what the rule was read from: per-tile bias partials and a row-count-only column sum
    for fn, needle in (("lstm_bwd_cluster.hip", "p.db_part[(size_t)tile *"), ("lstm_bwd8.hip", "p.db_part[(size_t)tile *"),
                       ("lstm_bwd16.hip", "p.db_part[(size_t)tile *"), ("reduce_defer.hip", "int chunks = (int)((rows + 127) / 128);"),
                       ("gemm_f32.hip", "const int cus = device_cu_count()")):
        with open(os.path.join(CSRC, fn)) as f:
            assert needle in f.read(), (fn, needle)


def test_every_round_taking_launcher_keeps_a_multi_round_case():
    kept = {}
    for r, limit, groups in rounds_cases():
        g = ROUNDS[r["rounds"]][1](r["H"])
        assert limit == groups * g and -(-ROUNDS_B // G.TILE) == 3 and ROUNDS_B % G.TILE == 1      # three tiles, one live row in the last
        kept.setdefault(r["rounds"], set()).add(groups)
    for launcher, (fn, _) in ROUNDS.items():
        assert os.path.exists(os.path.join(CSRC, fn))
        if launcher in UNREACHABLE_ROUNDS:
            assert launcher not in kept, launcher + ": reachable after all - take it out of UNREACHABLE_ROUNDS"
            continue
        assert kept.get(launcher) == {1, 2}, (launcher, kept.get(launcher))
    assert all(why for _, _, why in dropped_pairs())
    # the shape tests the dropped pairs were read from are still there
    for fn, needle in (("lstm_wide16.hip", "if (tiles > 8 || tiles > max_groups) return false;"),
                       ("lstm_bwd16.hip", "return !off && tiles >= 1 && tiles <= 8 && tiles <= cus / (H / 16);"),
                       ("lstm_bwd16.hip", "p.num_tiles <= device_cu_count() / 32) return launch_bwd16_t<512, 32>")):
        with open(os.path.join(CSRC, fn)) as f:
            assert needle in f.read(), (fn, needle)


def test_epoch_bases():
    """An odd base, an even one, one with high bits set below the re-zero threshold, and one the first launch crosses."""
    assert EPOCH_BASES[0] % 2 == 1 and EPOCH_BASES[1] == 2 and EPOCH_BASES[2] >> 28 and EPOCH_BASES[2] + 1000 < REZERO_ABOVE
    T = SHAPES[0][1]            # xch_account adds span + 2 before it compares; the smallest span of a row is T + 1 (one round)
    assert EPOCH_BASES[3] < REZERO_ABOVE < EPOCH_BASES[3] + (T + 1) + 2
    with open(os.path.join(CSRC, "api_state.hip")) as f:
        assert "if (st.epoch > 0x70000000ull)" in f.read()
    with open(os.path.join(CSRC, "xch_common.h")) as f:
        src = f.read()
    assert "ST_LAUNCHES = 2" in src and "ST_EPOCH = 3" in src and "ST_TIMEOUT = 0" in src
    assert "kXchBytes = (size_t)64 << 20" in src and "kArriveWords = 64" in src and "kArriveStride = 32" in src
