#!/usr/bin/env python3
"""Static VALU budget of one kernel by source region, from a build with line tables (make hip HIP_EXTRA=-gline-tables-only,
which must give the same instruction count as the shipped build: the line tables do not change the code).

Every instruction is mapped to its full inline chain (llvm-symbolizer --inlining) and put in a region of k_pool: the node step
(trav_node_step), the leaf visit / triangle test (trav_leaf), the shade pass split into its parts (shade_entry_on, by its
step), or a phase of the main loop by the kernels_pool.h line it came from.

    python tools/valu_budget.py LIB.so ["k_pool<256, 5, false, true, false, false, false, 0, false, true>"]
        [--times REGION=COUNT ...] [--regions TABLE.json] [--measured VALU] [--dump-static OUT.json]
    python tools/valu_budget.py --static STATIC.json --regions TABLE.json [--measured VALU]

--times gives a region's dynamic count (wave-level executions, e.g. trace.node_step=27.57e6 from the COUNT kernel's
wave_node_steps); the regions given are multiplied out and set against --measured (SQ_INSTS_VALU per launch).  A region's
static count is an upper bound of one execution: branches inside it that a wave skips are counted all the same.

--regions joins the static counts with the DYNAMIC table of a COUNT render of the same frame (prt_get_region_stats, written
as JSON {"region name of capi.REGION_NAMES": [wave-level executions, active lanes], ...}): every static region is multiplied
by the executions of the counter TIMES_OF names for it.  What --measured leaves over is printed as a region of its own.
--static / --dump-static: the static counts as JSON {region: VALU}, so that the join runs without the library.
"""
import collections, json, os, re, subprocess, sys, tempfile

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


# static region -> the counter whose wave-level executions multiply it (or (counter, scale): the three pushes of the 4-wide node
# step are one static region and are counted one by one, so one execution of the counter stands for a third of the region).  Code that every lane of a pass runs whatever it holds
# (list appends by ballot rank, loop heads) goes by the pass; code under a branch goes by that branch's counter.
TIMES_OF = {
    "entry": "wave", "exit": "wave",
    "topup.round": "round", "topup.pass": "topup_pass",
    "trace.setup": "round", "trace.outer": "trace_outer", "trace.refill": "refill", "trace.walk_pass": "walk_pass",
    "trace.node_loop": "node_step", "trace.node_step": "node_step", "trace.node_step.descend": "node_descend",
    "trace.node_step.pop": "node_pop", "trace.node_step.push": ("node_push", 1.0 / 3.0), "trace.finish.park": "park", "trace.leaf_visit": "leaf", "trace.leaf_tri": "tri", "trace.finish": "finish",
    "shade.setup": "round", "shade.end": "round", "shade.pass.loop": "shade_pass", "shade.pass.state_load": "shade_pass",
    "shade.pass.unattributed": "shade_pass", "shade.pass.step1": "shade_pass", "shade.pass.hit": "shade_hit",
    "shade.pass.miss": "shade_miss", "shade.pass.radiance_store": "radiance_store", "shade.pass.light": "shadow_block",
    "shade.pass.shadow_emit": "shade_pass", "shade.pass.walk.loop": "walk_loop", "shade.pass.walk.next_child": "walk_next_child",
    "shade.pass.walk.enter": "walk_enter", "shade.pass.walk.return_up": "walk_return_up", "shade.pass.walk.child_ray": "walk_child_ray", "shade.pass.outputs_emit": "shade_pass",
    # the fork step (forking kernels only): its test, draws and descriptor writes by the pass - an upper bound, a pass that does
    # not fork skips them -, its ray block by its own counter
    "shade.pass.fork": "shade_pass", "shade.pass.fork.leaf_ray": "leaf_ray",
}


def join(static, table, measured=None):
    """static {region: VALU of one execution}, table {counter: [executions, lanes]} -> (rows, total, rest): rows of
    (region, valu, counter, executions, mean active lanes, product), their sum, and measured - sum (None without `measured`).
    A static region without an entry in TIMES_OF, or whose counter the table lacks, is an error: nothing is dropped."""
    rows, total = [], 0.0
    for r in sorted(static):
        c = TIMES_OF.get(r)
        scale = 1.0
        if isinstance(c, tuple):
            c, scale = c
        if c is None or c not in table:
            raise KeyError("region %s: no counter (%s)" % (r, c))
        n, lanes = table[c][0], table[c][1]
        prod = float(static[r]) * float(n) * scale
        total += prod
        rows.append((r, static[r], c, n, (float(lanes) / n) if n else 0.0, prod))
    return rows, total, (None if measured is None else float(measured) - total)


def print_join(static, table, measured):
    rows, total, rest = join(static, table, measured)
    print("%-30s %6s  %-16s %12s %6s %12s %6s" % ("region", "valu", "x counter", "executions", "lanes", "valu x times", "share"))
    base = float(measured) if measured else total
    for r, v, c, n, fill, prod in rows:
        print("%-30s %6d  %-16s %12d %6.1f %12.4e %5.1f%%" % (r, v, c, n, fill, prod, 100.0 * prod / base))
    print("%-30s %6s  %-16s %12s %6s %12.4e %5.1f%%" % ("sum of the regions", "", "", "", "", total, 100.0 * total / base))
    if measured:
        print("%-30s %6s  %-16s %12s %6s %12.4e %5.1f%%" % ("not accounted (measured - sum)", "", "", "", "", rest, 100.0 * rest / base))
        print("measured SQ_INSTS_VALU per launch: %.4e; the regions sum to %.1f %% of it" % (measured, 100.0 * total / measured))


def regions(root):
    pool = os.path.join(root, "par_raytracer_amd", "csrc", "kernels_pool.h")
    wave = os.path.join(root, "par_raytracer_amd", "csrc", "kernels_wave.h")
    trav = os.path.join(root, "par_raytracer_amd", "csrc", "dev_trace4.h")
    p_loop, p_cam, p_cam_end, p_trace, p_refill, p_fill, p_fill_end, p_walk, p_nodes, p_nodes_end, p_fin, p_park, p_park_end, p_fin_end, p_shade, p_pass, p_ahead, p_ctr = _lines_of(pool, [
        "// ---- top up: fresh samples", "for (unsigned int k = ulane; k < cnt; k += ULANES) {", "n_c += cnt;",
        "// ---- trace: every ray of the pool", "const unsigned long long idle = __ballot(ray < 0);",
        "if (idle != 0ull && !dry) {", "const int leave_below = dry ? 1 : keep_min;",
        "while (ray >= 0) {", "while (trav_walking(r)) {", "bool fin = trav_done(r);", "if (fin) {",
        "if (!EXACT && trav_needs_slow_path(r, stack)) {", "hits[ray] = make_float4(r.best.t, r.best.v, r.best.w,",
        "if (__popcll(__ballot(true)) < leave_below) break;",
        "// ---- shade: every closest hit of the pool", "for (unsigned int b0 = b_first; b0 < n_c; b0 += ULANES)",
        "// ---- start ahead:", "// ---- counters: one atomic per workgroup"])
    w_on, w_step1, w_miss, w_hit, w_store, w_shadow, w_light, w_dead, w_fork, w_leaf_ray, w_leaf_ray_end, w_walk, w_child, w_enter, w_up, w_out, w_ray, w_emit = _lines_of(wave, [
        "PRT_D void shade_entry_on(", "// ---- step 1: the hit", "if (hit.tri < 0) {", "} else {", "write the record back",
        "// ---- shadow rays of this hit", "if (want_shadow) {", "// A shadow ray whose radiance-if-unoccluded is exactly zero",
        "// ---- fork: the children of a frame", "emit.region(PRT_REGION_LEAF_RAY);", "emit.closest(have, s_src,",
        "// ---- step 2: walk the bounce tree", "if (mode == M_NEXT_CHILD) {", "if (mode == M_ENTER) {", "if (mode == M_RETURN_UP) {",
        "// ---- outputs", "// ---- the child that flies", "// ---- append the next ray"])
    t_step, t_descend, t_pop, t_leaf, t_tris, t_tris_end = _lines_of(trav, [
        "PRT_D void trav_node_step(", "if (key[0] < inf) {", "} else {", "PRT_D bool trav_leaf(",
        "for (unsigned int i = 0; i < count; ++i) {", "if (flagged && r.sp == 1)"])

    def classify(frames):
        names = [f[0] for f in frames]
        if any("trav_node_step" in n for n in names):
            ln = max([f[2] for f in frames if f[1] == "dev_trace4.h" and t_step <= f[2] < t_leaf] or [0])
            if any("trav_push" in n or "::push" in n for n in names):
                return "trace.node_step.push"
            return "trace.node_step.descend" if t_descend <= ln < t_pop else "trace.node_step.pop" if ln >= t_pop else "trace.node_step"
        if any("trav_leaf" in n for n in names):
            ln = max([f[2] for f in frames if f[1] == "dev_trace4.h" and f[2] >= t_leaf] or [0])
            return "trace.leaf_tri" if (t_tris <= ln < t_tris_end or ln == 0) else "trace.leaf_visit"
        if any("shade_entry_on" in n for n in names):
            # the kernels_wave.h line inside shade_entry_on's body (0 = no line: code the compiler merged)
            ln = 0
            for f in frames:
                if f[1] == "kernels_wave.h" and w_on <= f[2] < w_emit + 4:
                    ln = f[2]
            if ln == 0:
                return "shade.pass.unattributed"
            if ln < w_step1:
                return "shade.pass.state_load"
            if ln < w_miss:
                return "shade.pass.step1"
            if ln < w_hit:
                return "shade.pass.miss"
            if ln < w_store:
                return "shade.pass.hit"
            if ln < w_shadow:
                return "shade.pass.radiance_store"
            if ln < w_light:
                return "shade.pass.shadow_emit"          # (the loop over the lights: every lane of the pass)
            if ln < w_dead:
                return "shade.pass.light"
            if ln < w_fork:
                return "shade.pass.shadow_emit"
            if ln < w_walk:
                return "shade.pass.fork.leaf_ray" if w_leaf_ray <= ln < w_leaf_ray_end else "shade.pass.fork"
            if ln < w_child:
                return "shade.pass.walk.loop"
            if ln < w_enter:
                return "shade.pass.walk.next_child"
            if ln < w_up:
                return "shade.pass.walk.enter"
            if ln < w_out:
                return "shade.pass.walk.return_up"
            return "shade.pass.walk.child_ray" if w_ray <= ln < w_emit else "shade.pass.outputs_emit"
        outer = frames[-1]
        kl = outer[2] if outer[1] == "kernels_pool.h" else 0
        if kl < p_loop:
            return "entry"
        if kl < p_trace:
            return "topup.pass" if p_cam <= kl < p_cam_end else "topup.round"
        if kl < p_refill:
            return "trace.setup"
        if kl < p_walk:
            return "trace.refill" if p_fill <= kl < p_fill_end else "trace.outer"
        if kl < p_shade:
            if p_nodes <= kl < p_nodes_end:
                return "trace.node_loop"
            if p_fin <= kl < p_fin_end:
                return "trace.finish.park" if p_park < kl < p_park_end - 1 else "trace.finish"
            return "trace.walk_pass" if kl < p_fin_end + 2 else "trace.outer"
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
    times, measured, table, static_in, static_out = {}, None, None, None, None
    for opt in ("--regions", "--static", "--dump-static"):
        if opt in args:
            i = args.index(opt); v = args[i + 1]; del args[i:i + 2]
            if opt == "--regions": table = json.load(open(v))
            elif opt == "--static": static_in = json.load(open(v))
            else: static_out = v
    if "--measured" in args:
        i = args.index("--measured"); measured = float(args[i + 1]); del args[i:i + 2]
    if "--times" in args:
        i = args.index("--times"); j = i + 1
        while j < len(args) and not args[j].startswith("--"):
            k, v = args[j].split("="); times[k] = float(v); j += 1
        del args[i:j]
    if static_in is not None:
        print_join(static_in, table, measured)
        return
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
        # basic blocks (a branch ends one, a branch target starts one): the node step's main block is the one with the byte ->
        # float converts; what the line tables give to the node step outside it runs under the push / pop branches
        base = int(body.split(" ", 1)[0], 16)
        targets = {base + int(t, 16) for t in re.findall(r"s_c?branch\S*\s.*?\+0x([0-9a-fA-F]+)>", body)}
        block, blocks, cvt_blocks, prev_branch = 0, [], set(), False
        for ln in body.split("\n")[1:]:
            m = re.match(r"^\s+([a-z_0-9]+)\b.*?//\s*([0-9A-Fa-f]+):", ln)
            if m:
                addr = int(m.group(2), 16)
                if addr in targets or prev_branch:
                    block += 1
                prev_branch = m.group(1).startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc"))
                if m.group(1).startswith("v_cvt_f32_ubyte"):
                    cvt_blocks.add(block)
                rows.append((addr, m.group(1)))
                blocks.append(block)
        out = subprocess.run([LLVM + "/llvm-symbolizer", "--obj=" + tmp + "/k.co", "--inlining", "--relative-address"],
                             input="\n".join("0x%x" % a for a, _ in rows), stdout=subprocess.PIPE, text=True, check=True).stdout
    chunks = out.strip("\n").split("\n\n")
    if len(chunks) != len(rows):
        sys.exit("symbolizer returned %d entries for %d instructions" % (len(chunks), len(rows)))
    classify = regions(root)
    agg = collections.defaultdict(lambda: [0, 0, 0, 0])
    for (_, ins), ch, blk in zip(rows, chunks, blocks):
        ls = ch.split("\n")
        frames = []
        for i in range(0, len(ls) - 1, 2):
            f = ls[i + 1].rsplit(":", 2)
            frames.append((ls[i], os.path.basename(f[0]), int(f[1]) if f[1].isdigit() else 0))
        region = classify(frames)
        if region == "trace.node_step" and blk not in cvt_blocks:
            region = "trace.node_step.push"
        g = agg[region]
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
    if static_out:
        json.dump({r: agg[r][1] for r in sorted(agg)}, open(static_out, "w"), indent=1)
    if table is not None:
        print()
        print_join({r: agg[r][1] for r in agg}, table, measured)
    if times:
        print("regions multiplied out: %.3e VALU" % dyn)
        if measured:
            print("measured: %.3e VALU; the regions given account for %.1f %%" % (measured, 100.0 * dyn / measured))


if __name__ == "__main__":
    main()
