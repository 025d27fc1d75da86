"""LDS waits between the MFMAs of k_commit_step's tiles, from the compiler's assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Iinclude \
        -o hdgnn.s hd-gnn_amd/csrc/hdgnn.hip
    python tools/mfma_waits.py hdgnn.s [kernel-name regex, default k_commit_step]
    python tools/mfma_waits.py --resources parent.s new.s     (every kernel symbol, side by side)

No GPU.  Per matching kernel symbol: registers, scratch, static LDS; then
  * per MFMA run (consecutive v_mfma lines of one basic block, at most GAP other instructions
    apart): the number of MFMAs and of `s_waitcnt ... lgkmcnt` lines between the first and the
    last of them, and the round trips among those: gaps between two MFMAs of the run in which
    an LDS read is issued and then waited for.  A batched 16-k-step body shows 4 MFMAs behind
    partial waits of the one read group issued before the first (descending counts, no round
    trip inside), a serialized one a read and a full wait before every MFMA;
  * in the instantiations that carry phase stamps (STAMPS = true, the third template
    argument), the same counts and the saveexec count per stamp interval n -> n+1, the numbers
    tools/mid_phases.py prints.  Stamp n is the s_memrealtime whose value is stored to
    stamps[prow * 32 + n], i.e. a global_store_dwordx2 with a scalar base and offset 8 n a
    few instructions later (the exchange's timeout reads and the per-wave stamps have other
    forms).  Intervals are in text order: the compiler keeps the phases' blocks in source order.
"""
import re
import sys

GAP = 24


def split_kernels(path):
    """name -> list of lines, from `name:` to the next kernel's label (code, descriptor and
    the compiler's resource comments)."""
    out, name, body = {}, None, []
    for raw in open(path):
        line = raw.rstrip("\n")
        m = re.match(r"^(\w+):\s*(;\s*@\1)?\s*$", line)
        if m and m.group(2):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is not None:
            body.append(line)
    return out


def insn(line):
    s = line.split(";")[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    return s


def lgkm(s):
    m = re.search(r"lgkmcnt\((\d+)\)", s)
    return int(m.group(1)) if s.startswith("s_waitcnt") and m else None


def report(name, body):
    meta = {}
    for line in body:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", line)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    print("== %s" % name)
    print("   " + "  ".join("%s %s" % (k.lstrip("."), v) for k, v in meta.items()))
    runs, cur, since, stamp, look = [], None, 0, -1, 0
    seg = {}
    for line in body:
        if line.strip().startswith(".amdhsa_kernel"):  # the descriptor: the code is over
            break
        if re.match(r"^\.?\w+:", line.strip()):      # label: a basic block boundary
            if cur:
                runs.append(cur)
            cur = None
            continue
        s = insn(line)
        if s is None:
            continue
        if s.startswith("s_memrealtime"):
            look = 12
        elif look > 0:
            look -= 1
            m = re.match(r"global_store_dwordx2 v\d+, v\[\d+:\d+\], s\[\d+:\d+\](?: offset:(\d+))?$", s)
            if m:
                stamp, look = int(m.group(1) or 0) // 8, 0
        c = seg.setdefault(stamp, dict(insn=0, mfma=0, waits=0, saveexec=0, ds=0))
        c["insn"] += 1
        w = lgkm(s)
        if s.startswith("v_mfma"):
            c["mfma"] += 1
            if cur is None or since > GAP:
                if cur:
                    runs.append(cur)
                cur = dict(stamp=stamp, mfma=0, waits=[], pend=[], rt=0, rd=False, hit=False)
            cur["mfma"] += 1
            cur["waits"] += cur["pend"]
            cur["rt"] += cur["hit"]
            cur["pend"], cur["rd"], cur["hit"] = [], False, False
            since = 0
            continue
        since += 1
        if w is not None:
            c["waits"] += 1
            if cur is not None:
                cur["pend"].append(w)
                cur["hit"] = cur["hit"] or cur["rd"]
        elif "saveexec" in s:
            c["saveexec"] += 1
        elif s.startswith("ds_read") or s.startswith("ds_load"):
            c["ds"] += 1
            if cur is not None:
                cur["rd"] = True
        if s.startswith("s_cbranch") or s.startswith("s_branch"):
            if cur:
                runs.append(cur)
            cur = None
    if cur:
        runs.append(cur)
    print("   MFMA runs: interval  mfmas  lds-waits-inside  round-trips-inside  (wait counts)")
    tot = dict(mfma=0, waits=0, groups=0)
    for r in runs:
        g = r["rt"]
        tot["mfma"] += r["mfma"]
        tot["waits"] += len(r["waits"])
        tot["groups"] += g
        print("     %2d->%-2d  %3d  %3d  %3d  (%s)" % (r["stamp"], r["stamp"] + 1, r["mfma"], len(r["waits"]), g,
                                                 " ".join(map(str, r["waits"]))))
    print("   runs %d: mfmas %d, lds waits inside runs %d, round trips inside %d" % (
        len(runs), tot["mfma"], tot["waits"], tot["groups"]))
    if stamp >= 0:
        print("   per stamp interval: insns  mfmas  ds_reads  lds-waits  saveexec")
        for k in sorted(seg):
            c = seg[k]
            print("     %2d->%-2d  %5d  %3d  %4d  %3d  %3d" % (k, k + 1, c["insn"], c["mfma"], c["ds"], c["waits"],
                                                          c["saveexec"]))
    else:
        c = seg[-1]
        print("   whole kernel: insns %d  mfmas %d  ds_reads %d  lds-waits %d  saveexec %d" % (
            c["insn"], c["mfma"], c["ds"], c["waits"], c["saveexec"]))


def resources(body):
    meta = {}
    for line in body:
        m = re.match(r"^; (NumVgprs|ScratchSize|LDSByteSize): (\d+)", line)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return meta.get("NumVgprs"), meta.get("ScratchSize"), meta.get("LDSByteSize")


def resource_table(a, b):
    ka, kb = split_kernels(a), split_kernels(b)
    print("VGPRs / scratch bytes / static LDS bytes per kernel symbol: %s | %s" % (a, b))
    worse = 0
    names = [n for n in sorted(set(ka) | set(kb))          # kernels: symbols with a descriptor
             if any(l.strip().startswith(".amdhsa_kernel") for l in ka.get(n, kb.get(n)))]
    for name in names:
        ra = resources(ka[name]) if name in ka else None
        rb = resources(kb[name]) if name in kb else None
        flag = ""
        if ra and rb and any(y > x for x, y in zip(ra, rb)):
            flag, worse = "  WORSE", worse + 1
        print("%s  %s | %s%s" % (name, ra, rb, flag))
    print("%d kernel symbols, %d worse" % (len(names), worse))


def main():
    if sys.argv[1] == "--resources":
        return resource_table(sys.argv[2], sys.argv[3])
    path = sys.argv[1]
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else "k_commit_step")
    ks = split_kernels(path)
    for name in sorted(ks):
        if pat.search(name):
            report(name, ks[name])


if __name__ == "__main__":
    main()
