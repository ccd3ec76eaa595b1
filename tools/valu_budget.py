#!/usr/bin/env python3
"""Static VALU budget of one kernel by source region, from a build with line tables (make hip HIP_EXTRA=-gline-tables-only,
which must give the same instruction count as the shipped build: the line tables do not change the code).

Every instruction is mapped to its full inline chain (llvm-symbolizer --inlining) and put in a region of k_pool: the node step
(trav_node_step), the leaf visit / triangle test (trav_leaf), the shade pass split into its parts (shade_entry_on, by its
step), or a phase of the main loop by the kernels_pool.h line it came from.

    python tools/valu_budget.py LIB.so ["k_pool<256, 5, false, true, false, false, false, 0, false, true>"]
        [--times REGION=COUNT ...] [--measured VALU]

--times gives a region's dynamic count (wave-level executions, e.g. trace.node_step=27.57e6 from the COUNT kernel's
wave_node_steps); the regions given are multiplied out and set against --measured (SQ_INSTS_VALU per launch).  A region's
static count is an upper bound of one execution: branches inside it that a wave skips are counted all the same.
"""
import collections, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"

# kernels_pool.h line ranges of k_pool's phases, and shade_entry_on's steps in kernels_wave.h: located from the source's own
# section comments so that the tool follows edits of the files
def _lines_of(path, marks):
    src = open(path).read().split("\n")
    out, at = [], 0
    for m in marks:                      # each marker is looked for after the one before it
        hit = [i + 1 for i, l in enumerate(src) if i >= at and m in l]
        if not hit:
            sys.exit("marker not found in %s: %r" % (path, m))
        out.append(hit[0])
        at = hit[0]
    return out


def regions(root):
    pool = os.path.join(root, "par_raytracer_amd", "csrc", "kernels_pool.h")
    wave = os.path.join(root, "par_raytracer_amd", "csrc", "kernels_wave.h")
    p_loop, p_trace, p_refill, p_walk, p_shade, p_pass, p_ahead, p_ctr = _lines_of(pool, [
        "// ---- top up: fresh samples", "// ---- trace: every ray of the pool", "const unsigned long long idle = __ballot(ray < 0);",
        "while (ray >= 0) {", "// ---- shade: every closest hit of the pool", "for (unsigned int b0 = b_first; b0 < n_c; b0 += ULANES)",
        "// ---- start ahead:", "// ---- counters: one atomic per workgroup"])
    w_on, w_step1, w_store, w_shadow, w_walk, w_out = _lines_of(wave, [
        "PRT_D void shade_entry_on(", "// ---- step 1: the hit", "write the record back", "// ---- shadow rays of this hit",
        "// ---- step 2: walk the bounce tree", "// ---- outputs"])

    def classify(frames):
        names = [f[0] for f in frames]
        if any("trav_node_step" in n for n in names):
            return "trace.node_step"
        if any("trav_leaf" in n for n in names):
            return "trace.leaf_tri"
        if any("shade_entry_on" in n for n in names):
            # the kernels_wave.h line inside shade_entry_on's body (0 = no line: code the compiler merged)
            ln = 0
            for f in frames:
                if f[1] == "kernels_wave.h" and w_on <= f[2] < w_out + 20:
                    ln = f[2]
            if ln == 0:
                return "shade.pass.unattributed"
            if ln < w_step1:
                return "shade.pass.state_load"
            if ln < w_store:
                return "shade.pass.hit"
            if ln < w_shadow:
                return "shade.pass.radiance_store"
            if ln < w_walk:
                return "shade.pass.shadow_rays"
            if ln < w_out:
                return "shade.pass.bounce_walk"
            return "shade.pass.outputs_emit"
        outer = frames[-1]
        kl = outer[2] if outer[1] == "kernels_pool.h" else 0
        if kl < p_loop:
            return "entry"
        if kl < p_trace:
            return "topup"
        if kl < p_refill:
            return "trace.setup"
        if kl < p_walk:
            return "trace.refill"
        if kl < p_shade:
            return "trace.loop_bookkeeping"
        if kl < p_pass:
            return "shade.setup"
        if kl < p_ahead:
            return "shade.pass.loop"
        if kl < p_ctr:
            return "shade.end"
        return "exit"
    return classify


def main():
    args = [a for a in sys.argv[1:]]
    times, measured = {}, None
    if "--measured" in args:
        i = args.index("--measured"); measured = float(args[i + 1]); del args[i:i + 2]
    if "--times" in args:
        i = args.index("--times"); j = i + 1
        while j < len(args) and not args[j].startswith("--"):
            k, v = args[j].split("="); times[k] = float(v); j += 1
        del args[i:j]
    so = args[0]
    want = args[1] if len(args) > 1 else "k_pool<256, 5, false, true, false, false, false, 0, false, true>"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, tmp + "/fat.bin"], check=True)
        subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--unbundle", "--input=" + tmp + "/fat.bin",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + tmp + "/k.co"], check=True)
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--demangle", "--no-show-raw-insn", tmp + "/k.co"],
                             stdout=subprocess.PIPE, check=True).stdout.decode()
        body = next((f for f in re.split(r"\n(?=[0-9a-f]{16} <)", dis) if want + "(" in f.split("\n", 1)[0]), None)
        if body is None:
            sys.exit("kernel not found: " + want)
        rows = []
        for ln in body.split("\n")[1:]:
            m = re.match(r"^\s+([a-z_0-9]+)\b.*?//\s*([0-9A-Fa-f]+):", ln)
            if m:
                rows.append((int(m.group(2), 16), m.group(1)))
        out = subprocess.run([LLVM + "/llvm-symbolizer", "--obj=" + tmp + "/k.co", "--inlining", "--relative-address"],
                             input="\n".join("0x%x" % a for a, _ in rows), stdout=subprocess.PIPE, text=True, check=True).stdout
    chunks = out.strip("\n").split("\n\n")
    if len(chunks) != len(rows):
        sys.exit("symbolizer returned %d entries for %d instructions" % (len(chunks), len(rows)))
    classify = regions(root)
    agg = collections.defaultdict(lambda: [0, 0, 0, 0])
    for (_, ins), ch in zip(rows, chunks):
        ls = ch.split("\n")
        frames = []
        for i in range(0, len(ls) - 1, 2):
            f = ls[i + 1].rsplit(":", 2)
            frames.append((ls[i], os.path.basename(f[0]), int(f[1]) if f[1].isdigit() else 0))
        g = agg[classify(frames)]
        g[0] += 1
        if ins.startswith("v_"):
            g[1] += 1
        if ins in ("v_readlane_b32", "v_writelane_b32"):
            g[2] += 1
        if ins.startswith("scratch_"):
            g[3] += 1
    print("%s: %d instructions, %d VALU" % (want, sum(g[0] for g in agg.values()), sum(g[1] for g in agg.values())))
    print("%-28s %6s %6s %10s %8s %14s" % ("region", "ins", "valu", "lane-spill", "scratch", "valu x times"))
    dyn = 0.0
    for r in sorted(agg):
        g = agg[r]
        t = times.get(r)
        extra = ""
        if t is not None:
            dyn += g[1] * t
            extra = "%14.3e" % (g[1] * t)
        print("%-28s %6d %6d %10d %8d %14s" % (r, g[0], g[1], g[2], g[3], extra))
    if times:
        print("regions multiplied out: %.3e VALU" % dyn)
        if measured:
            print("measured: %.3e VALU; the regions given account for %.1f %%" % (measured, 100.0 * dyn / measured))


if __name__ == "__main__":
    main()
