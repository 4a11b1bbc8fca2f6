"""Diagnostic: instruction counts by class for every MFMA-carrying loop of one kernel in hipcc's assembly - what a step of
the cluster LSTM kernel issues besides its MFMAs (with one wave per SIMD every VALU instruction, taken branch and exec-mask
switch is paid in full).  Loops are the strongly connected components of the kernel's basic-block
graph, and inside each, again, those left when the edges back to its entry block are cut (hipcc does not lay the blocks of
a loop out in one piece, so label order says nothing); the instructions of an inner MFMA-carrying loop are counted with
that loop only.  Classes go by mnemonic prefix alone.
usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --offload-device-only -o k.s lstm_cluster.hip
       python tools/isa_step_counts.py k.s [kernel-name substring, default the H = 256 sigmoid fused kernel that loads R from packs; ...ELb0: the one that does not] [--hist]
--hist adds each loop's non-MFMA mnemonics with their counts."""
import re
import sys

CLASSES = ["mfma", "valu", "branch", "exec", "salu", "lds", "vmem", "wait", "other"]
MIN_MFMA = 64   # spin loops and the like carry none


def classify(op, args):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op in ("s_barrier", "s_sleep", "s_endpgm"):
        return "other"
    if op.startswith("s_"):
        return "exec" if ("saveexec" in op or args.startswith("exec")) else "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def kernel_body(lines, sub):
    body, name = [], None
    for l in lines:
        t = l.split(";")[0].split("//")[0].strip()
        m = re.match(r"^(_Z\w+):", t)
        if m:
            name = m.group(1)
            continue
        if t.startswith(".Lfunc_end"):
            name = None
        if name is None or sub not in name:
            continue
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(t)
    return body


def basic_blocks(body):
    """-> blocks: list of lists of (op, args); succ: list of sets of block numbers; names: first label of each block"""
    blocks, names, label_block = [[]], ["entry"], {}
    for t in body:
        if t.endswith(":"):
            if blocks[-1]:
                blocks.append([])
                names.append(t[:-1])
            elif names[-1] == "entry" or not names[-1].startswith(".LBB"):
                names[-1] = t[:-1]
            label_block[t[:-1]] = len(blocks) - 1
            continue
        parts = t.split(None, 1)
        op, args = parts[0], (parts[1].strip() if len(parts) > 1 else "")
        blocks[-1].append((op, args))
        if classify(op, args) == "branch" or op == "s_endpgm":
            blocks.append([])
            names.append("(after %s)" % names[-1])
    succ = []
    for b, ins in enumerate(blocks):
        s = set()
        last = ins[-1] if ins else ("", "")
        if last[0].startswith(("s_cbranch", "s_branch")) and last[1] in label_block:
            s.add(label_block[last[1]])
        if not last[0].startswith("s_branch") and last[0] != "s_endpgm" and b + 1 < len(blocks):
            s.add(b + 1)
        succ.append(s)
    return blocks, succ, names


def sccs(nodes, succ):
    """Tarjan, iterative; -> components (sets) that hold a cycle"""
    nodes = set(nodes)
    index, low, on, stack, out, n = {}, {}, set(), [], [], [0]
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter(sorted(succ[root] & nodes)))]
        index[root] = low[root] = n[0]; n[0] += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n[0]; n[0] += 1; stack.append(w); on.add(w)
                    work.append((w, iter(sorted(succ[w] & nodes))))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = set()
                    while True:
                        w = stack.pop(); on.discard(w); comp.add(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(comp)
    return out


def main():
    argv = [a for a in sys.argv[1:] if a != "--hist"]
    hist = "--hist" in sys.argv
    sub = argv[1] if len(argv) > 1 else "lstm_cluster_fused_kernelILi256ELi0ELb1"
    body = kernel_body(open(argv[0]).read().split("\n"), sub)
    if not body:
        sys.exit("no kernel matches %r" % sub)
    blocks, succ, names = basic_blocks(body)
    pred = [set() for _ in blocks]
    for b, s in enumerate(succ):
        for w in s:
            pred[w].add(b)
    nmfma = [sum(op.startswith("v_mfma") for op, _ in ins) for ins in blocks]
    found = []   # (entry block, blocks, depth)

    def walk(nodes, edges, depth):
        for comp in sccs(nodes, edges):
            if sum(nmfma[b] for b in comp) < MIN_MFMA:
                continue
            heads = sorted(b for b in comp if pred[b] - comp) or [min(comp)]
            found.append((heads[0], comp, depth))
            cut = [s - set(heads) if b in comp else s for b, s in enumerate(edges)]
            walk(comp, cut, depth + 1)

    walk(range(len(blocks)), succ, 0)
    print("kernel *%s*: %d instructions, %d MFMA-carrying loop(s)" % (sub, sum(len(b) for b in blocks), len(found)))
    for head, comp, depth in sorted(found, key=lambda f: f[0]):
        inner = [c for h, c, d in found if d == depth + 1 and c < comp]
        own = comp - set().union(*inner) if inner else comp
        counts, ops = dict.fromkeys(CLASSES, 0), {}
        for b in own:
            for op, args in blocks[b]:
                counts[classify(op, args)] += 1
                ops[op] = ops.get(op, 0) + 1
        print("%sloop at %s, %d blocks%s: " % ("  " * depth, names[head], len(own), " (without its %d inner loop(s))" % len(inner) if inner else "")
              + "  ".join("%s %d" % (c, counts[c]) for c in CLASSES))
        if hist:
            print("%s    " % ("  " * depth) + ", ".join("%s %d" % (o, k) for o, k in sorted(ops.items(), key=lambda x: -x[1]) if not o.startswith("v_mfma")))


if __name__ == "__main__":
    main()
