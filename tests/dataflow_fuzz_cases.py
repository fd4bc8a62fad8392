"""Seeded random lowered FUNCTIONS (no GPU needed): where the kernels of a func.func read and write.

The other fuzz files draw kernels; this one draws the dataflow around them -- the part the emitter (emit_function /
emit_group: dest_of, returned_producer, nothing_observes_between) and the host runtime (Scope::bind_memref, place_result,
writes_direct, overlaps, run_store, finish, export_result) decide.  One module = one element type, a MAIN box with a logical
origin away from 0 and a WIDE box around it (0-3 extra cells per side, asymmetric), three or four opdefs from
test_fuzz_gpu.gen_apply on the main box (the last one holds two applies, the second consuming the first) and two or three
func.func over 3-5 memref arguments, each wrapped into a field of the main or of the wide box.  A body is a straight line of

    load (also of a field stored to earlier: a load is an alias, not a snapshot) | apply_nonlinear of an opdef on loaded
    temps and earlier results | two adjacent inline neptune_ir.apply over shared inputs (a group, where the union footprint
    allows one) | explicit time_advance (f64, where an opdef takes one input) | store without bounds | store with bounds
    (a sub-box, an empty box, the whole common box; between boxes of different origin; of a LOADED temp, i.e. field to
    field; into a field already stored to) | reduce (sum) over a declared box as the scalar result

and returns the unwrap of any argument's field, a computed temp, the scalar, or nothing.  Rank 4 lifts gen_apply's rank-3
stencils by one leading (batch) dimension: one rank-3 launch, store-box copy and reduce per leading index.

Left out because the reference leaves it undefined or the runtime refuses it by design: accesses outside a box, store or
reduce bounds that leave a buffer, more than one result, solver ops, and buffers that overlap without being identical
(memref.copy between partially overlapping views is not defined).  A reduce never takes a single-use inline apply: that
form is evaluated inside the reduction kernel and has its own tests (tests/test_reduce_exact_gpu.py)."""
import re

import numpy as np

import helpers
from test_fuzz_gpu import gen_apply

SEEDS = [1, 3, 9, 11, 13, 14, 21, 22, 23, 45, 68, 81]

BINDINGS = ("device", "host", "mixed", "aliased-device", "aliased-host")


def _bnd(lb, ub):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, lb))}], ub = [{', '.join(map(str, ub))}]>"


_BND_RE = re.compile(r"#neptune_ir\.bounds<lb = \[([^\]]*)\], ub = \[([^\]]*)\]>")


def _lift(text, lb0, ub0):
    """a rank-3 opdef of gen_apply -> rank 4: no offset along the new leading dimension, its bounds [lb0, ub0)"""
    text = re.sub(r"(neptune_ir\.access %in\d+\[)", r"\g<1>0, ", text)
    text = text.replace("^bb0(%i0: index", "^bb0(%lead: index, %i0: index")
    return text.replace("lb = [", f"lb = [{lb0}, ").replace("ub = [", f"ub = [{ub0}, ")


def _apply_lines(text):
    """the neptune_ir.apply of a gen_apply opdef (its lines without the opdef's header, return and brace) and its bounds"""
    lines = text.split("\n")[2:-2]
    m = _BND_RE.search(lines[0])
    return lines, ([int(x) for x in m.group(1).split(",")], [int(x) for x in m.group(2).split(",")])


def _rebind(lines, result, operands, bounds=None):
    """that apply with another result name and operands (and bounds)"""
    first = re.sub(r"%r = neptune_ir\.apply\([^)]*\)", f"{result} = neptune_ir.apply({', '.join(operands)})", lines[0])
    if bounds is not None:
        first = _BND_RE.sub(_bnd(*bounds), first)
    return [first] + lines[1:]


def _sub_box(rng, box, kind):
    """a store / reduce box inside `box`: "full", "sub" (0-2 cells off each side, 0-3 along the rows) or "empty" (one axis
    of extent 0, somewhere inside)"""
    lb, ub = list(box[0]), list(box[1])
    if kind == "full":
        return lb, ub
    rank = len(lb)
    for d in range(rank):
        most = 3 if d == rank - 1 else 2
        lb[d] += int(rng.integers(0, most + 1))
        ub[d] -= int(rng.integers(0, most + 1))
    if kind == "empty":
        d = int(rng.integers(0, rank))
        lb[d] = ub[d] = int(rng.integers(lb[d], ub[d] + 1))
    return lb, ub


def gen_dataflow_module(seed):
    """-> (module text, meta).  meta: rank, elem, main / wide boxes, ops [(name, nin)] and per function its argument kinds,
    result kind, the reads and writes of its arguments in program order, and feature counts (see features())"""
    rng = np.random.default_rng(seed)
    rank = int(rng.choice([1, 2, 2, 3, 3, 3, 4]))
    elem = str(rng.choice(["f64", "f32"]))
    last = int(rng.choice([130, 131, 260, 261]))
    if elem == "f32":
        last = 2 * last + int(rng.integers(0, 4))
    shape = [int(rng.integers(6, 13)) for _ in range(rank - 1)] + [last]
    origin = [int(rng.choice([-3, -2, -1, 1, 2, 3, 4])) for _ in range(rank)]
    lo = [int(rng.integers(0, 4)) for _ in range(rank)]
    hi = [int(rng.integers(0, 4)) for _ in range(rank)]
    d = int(rng.integers(0, rank))
    hi[d] = (lo[d] + 1 + int(rng.integers(0, 3))) % 4                     # asymmetric along one axis at least
    main = (tuple(origin), tuple(o + n for o, n in zip(origin, shape)))
    wide = (tuple(o - a for o, a in zip(origin, lo)), tuple(u + b for u, b in zip(main[1], hi)))
    boxes = {"main": main, "wide": wide}
    head = ['#l = #neptune_ir.location<"cell">', f"#b = {_bnd(*main)}", f"#bw = {_bnd(*wide)}",
            f"!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>",
            f"!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>",
            f"!tw = !neptune_ir.temp<element = {elem}, bounds = #bw, location = #l>",
            f"!fw = !neptune_ir.field<element = {elem}, bounds = #bw, location = #l>", "module {"]
    TEMP, FIELD = {"main": "!t", "wide": "!tw"}, {"main": "!f", "wide": "!fw"}

    def raw_apply(name):
        if rank < 4:
            return gen_apply(rng, name, rank, elem, shape, origin)
        text, nin = gen_apply(rng, name, 3, elem, shape[1:], origin[1:])
        return _lift(text, origin[0] + int(rng.integers(0, 2)), main[1][0] - int(rng.integers(0, 2))), nin

    # ---- opdefs: op0.. from gen_apply, the last one two applies, the second consuming the first
    nops = int(rng.integers(3, 5))
    ops = []
    for n in range(nops - 1):
        text, nin = raw_apply(f"op{n}")
        head.append(text)
        ops.append((f"op{n}", nin))
    (ta, na), (tb, nb) = raw_apply("a"), raw_apply("b")
    la, _ = _apply_lines(ta)
    lb_, _ = _apply_lines(tb)
    nin2 = max(na, nb)
    name2 = f"op{nops - 1}"
    head += [f"  neptune_ir.nonlinear_opdef @{name2} : ({', '.join(['!t'] * nin2)}) -> !t {{",
             "  ^bb0(" + ", ".join(f"%u{k}: !t" for k in range(nin2)) + "):"]
    head += _rebind(la, "%r0", [f"%u{k}" for k in range(na)])
    head += _rebind(lb_, "%r", ["%r0"] + [f"%u{k}" for k in range(1, nb)])
    head += ["    neptune_ir.return %r : !t", "  }"]
    ops.append((name2, nin2))
    rhs = [name for name, nin in ops if nin == 1]

    mr = "x".join("?" * rank) + "x" + elem
    functions = []
    for fi in range(int(rng.integers(2, 4))):
        fname = f"fn{fi}"
        nargs = int(rng.integers(3, 6))
        kinds = ["main", "main"] + [("wide" if rng.random() < 0.4 else "main") for _ in range(nargs - 2)]
        kinds = [kinds[i] for i in rng.permutation(nargs)]
        B = [f"    %f{k} = neptune_ir.wrap %m{k} : memref<{mr}> -> {FIELD[kinds[k]]}" for k in range(nargs)]
        temps = []          # dicts: name, kind, root (argument it aliases, or None), how (load | call | inline | ta), uses
        stored = set()
        stores = []
        events = []         # (what, argument) in program order: "r" a kernel reads it, "w" a store writes it
        feat = dict.fromkeys(("load_after_store", "diff_origin", "empty_store", "field_to_field", "second_store",
                              "inline_pair", "time_advance", "bounded_store", "full_store", "inplace_forward",
                              "observed_between"), 0)
        cnt = [0]

        def new_temp(kind, root, how, ins=()):
            cnt[0] += 1
            t = dict(name=f"%t{cnt[0]}", kind=kind, root=root, how=how, uses=0, pos=len(B),
                     in_roots={i["root"] for i in ins if i["root"] is not None})
            temps.append(t)
            return t

        def use(t):
            t["uses"] += 1
            if t["root"] is not None:
                events.append(("r", t["root"], len(B)))

        def call(ins, name=None):
            if name is None:
                name = [n for n, nin in ops if nin == len(ins)][0]
            for t in ins:
                use(t)
            r = new_temp("main", None, "call", ins)
            B.append(f"    {r['name']} = neptune_ir.apply_nonlinear @{name}(" + ", ".join(t["name"] for t in ins) + ") : (" +
                     ", ".join(["!t"] * len(ins)) + ") -> !t")
            return r

        def load(k):
            t = new_temp(kinds[k], k, "load")
            B.append(f"    {t['name']} = neptune_ir.load %f{k} : {FIELD[kinds[k]]} -> {TEMP[kinds[k]]}")
            feat["load_after_store"] += k in stored
            return t

        def pick_inputs(n):
            pool = [t for t in temps if t["kind"] == "main"]
            recent = [t for t in pool if t["how"] != "load"][-2:]
            out = []
            for _ in range(n):
                out.append(recent[int(rng.integers(0, len(recent)))] if recent and rng.random() < 0.4
                           else pool[int(rng.integers(0, len(pool)))])
            return out

        def store(bounded, src=None, k=None):
            loaded = [t for t in temps if t["how"] == "load"]
            computed = [t for t in temps if t["how"] != "load"]
            if src is not None:
                pass
            elif computed and (not loaded or rng.random() < 0.75):
                src = computed[-1] if rng.random() < 0.7 else computed[int(rng.integers(0, len(computed)))]
            else:
                src = loaded[int(rng.integers(0, len(loaded)))]
            cands = [j for j in range(nargs) if bounded or kinds[j] == src["kind"]]
            again = [j for j in cands if j in stored]
            if k is None:
                k = again[int(rng.integers(0, len(again)))] if again and rng.random() < 0.4 else cands[int(rng.integers(0, len(cands)))]
            attr = ""
            if bounded:
                common = main if "main" in (src["kind"], kinds[k]) else wide
                how = str(rng.choice(["sub", "sub", "sub", "empty", "full"]))
                b = _sub_box(rng, common, how)
                attr = f" {{bounds = {_bnd(*b)}}}"
                feat["empty_store"] += how == "empty"
                feat["bounded_store"] += 1
                feat["diff_origin"] += boxes[src["kind"]][0] != boxes[kinds[k]][0]
            else:
                feat["full_store"] += 1
            feat["field_to_field"] += src["how"] == "load"
            feat["second_store"] += k in stored
            use(src)
            B.append(f"    neptune_ir.store {src['name']} to %f{k}{attr} : {TEMP[src['kind']]} to {FIELD[kinds[k]]}")
            events.append(("w", k, len(B)))
            stores.append(dict(src=src, k=k, bounded=bounded, pos=len(B)))
            stored.add(k)

        load(int(rng.choice([k for k in range(nargs) if kinds[k] == "main"])))
        nstores = 0
        for _ in range(int(rng.integers(4, 10)) - 1):
            what = str(rng.choice(["load", "load", "call", "call", "call", "inline", "ta", "store", "store", "box", "box", "box", "observe", "forward", "hazard"]))
            if what == "load":
                load(int(rng.integers(0, nargs)))
            elif what == "call":
                name, nin = ops[int(rng.integers(0, len(ops)))]
                call(pick_inputs(nin), name)
            elif what == "forward":
                # y = A(...) and its whole-field store right behind it: the field goes down to A as its destination, which
                # may use it unless the field is one of A's own inputs
                name, nin = ops[int(rng.integers(0, len(ops)))]
                store(False, call(pick_inputs(nin), name))
                nstores += 1
            elif what == "observe":
                # y = A(...) away from field k, then z = B(load fk, ...), then store y to fk: y may not be written into fk
                # where it is produced, z still reads the old fk
                mains = [j for j in range(nargs) if kinds[j] == "main"]
                k, other = (int(j) for j in rng.permutation(mains)[:2])
                tk = next((t for t in temps if t["root"] == k), None) or load(k)
                away = [t for t in temps if t["kind"] == "main" and t["root"] != k] or [load(other)]
                name, nin = ops[int(rng.integers(0, len(ops)))]
                y = call([away[int(rng.integers(0, len(away)))] for _ in range(nin)], name)
                name, nin = ops[int(rng.integers(0, len(ops)))]
                z = call([tk] + pick_inputs(nin - 1), name)
                store(False, y, k)
                store(bool(rng.random() < 0.5), z, other)                   # ... and z is looked at
                nstores += 2
            elif what == "hazard":
                # y = an inline apply reading field a, stored whole into field b right behind it, then a is read again:
                # with a and b ONE buffer the apply may not write where it reads (the runtime compares the pointers), and
                # the later read sees y
                mains = [j for j in range(nargs) if kinds[j] == "main"]
                a, b = (int(j) for j in rng.permutation(mains)[:2])
                ta = next((t for t in temps if t["root"] == a), None) or load(a)
                text1, n1 = raw_apply("h")
                ins = [ta] + pick_inputs(n1 - 1)
                for t in ins:
                    use(t)
                y = new_temp("main", None, "inline", ins)
                B += ["    " + s_.lstrip() for s_ in _rebind(_apply_lines(text1)[0], y["name"], [t["name"] for t in ins])]
                store(False, y, b)
                name, nin = ops[int(rng.integers(0, len(ops)))]
                z = call([ta] + pick_inputs(nin - 1), name)
                store(bool(rng.random() < 0.5), z)
                nstores += 2
            elif what == "inline":
                # two sibling applies over a small pool of shared inputs, on one apply.bounds (the intersection: tighter
                # bounds keep every access in range)
                (t1, n1), (t2, n2) = raw_apply("x"), raw_apply("y")
                (l1, b1), (l2, b2) = _apply_lines(t1), _apply_lines(t2)
                both = ([max(a, b) for a, b in zip(b1[0], b2[0])], [min(a, b) for a, b in zip(b1[1], b2[1])])
                pool = pick_inputs(int(rng.integers(1, 4)))
                pair = []
                for l, n in ((l1, n1), (l2, n2)):
                    ins = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
                    for t in ins:
                        use(t)
                    r = new_temp("main", None, "inline", ins)
                    B += ["    " + s.lstrip() for s in _rebind(l, r["name"], [t["name"] for t in ins], both)]
                    pair.append(r)
                feat["inline_pair"] += 1
                # ... and, half of the time, their whole-field stores right behind them: a member may write into its field
                for r in pair[:int(rng.integers(0, 3))] if rng.random() < 0.5 else []:
                    store(False, r)
                    nstores += 1
            elif what == "ta":
                if elem != "f64" or not rhs:            # the explicit time_advance is f64 and takes rhs(state)
                    continue
                state = pick_inputs(1)[0]
                use(state)
                r = new_temp("main", None, "ta", [state])
                B += [f"    %dt{cnt[0]} = arith.constant {float(rng.choice([0.125, -0.25, 0.5]))!r} : f64",
                      f"    {r['name']} = neptune_ir.time_advance {state['name']}, %dt{cnt[0]} {{method = 0 : i32, rhs = @{rhs[0]}}} : !t, f64 -> !t"]
                feat["time_advance"] += 1
            else:
                store(what == "box")
                nstores += 1
        if nstores == 0:
            store(bool(rng.random() < 0.5))
        # ---- the result
        computed = [t for t in temps if t["how"] != "load"]
        result = str(rng.choice(["unwrap", "unwrap", "temp", "temp", "scalar", "none"]))
        if result == "temp" and not computed:
            result = "unwrap"
        fn = dict(name=fname, kinds=kinds, result=result, result_arg=None, reduce=None)
        if result == "unwrap":
            k = int(rng.integers(0, nargs))
            fn["result_arg"] = k
            B += [f"    %res = neptune_ir.unwrap %f{k} : {FIELD[kinds[k]]} -> memref<{mr}>", f"    func.return %res : memref<{mr}>"]
            rty = f" -> memref<{mr}>"
        elif result == "temp":
            t = computed[-1] if rng.random() < 0.5 else computed[int(rng.integers(0, len(computed)))]
            t["uses"] += 1
            B.append(f"    func.return {t['name']} : !t")
            rty = " -> !t"
        elif result == "scalar":
            cands = [t for t in temps if t["how"] != "inline"]
            t = cands[int(rng.integers(0, len(cands)))]
            b = _sub_box(rng, boxes[t["kind"]], str(rng.choice(["sub", "sub", "full"])))
            use(t)
            fn["reduce"] = dict(kind=t["kind"], box=b)
            B += [f"    %s = neptune_ir.reduce {t['name']} in {_bnd(*b)} {{kind = \"sum\"}} : {TEMP[t['kind']]} -> {elem}",
                  f"    func.return %s : {elem}"]
            rty = f" -> {elem}"
        else:
            B.append("    func.return")
            rty = ""
        head += [f"  func.func @{fname}(" + ", ".join(f"%m{k}: memref<{mr}>" for k in range(nargs)) + f"){rty} {{"] + B + ["  }"]
        # unbounded stores of a single-use computed temp: the emitter may hand the field down to the producer
        hazards = []        # (a, k): the producer reads argument a and its result goes to field k
        for st in stores:
            y = st["src"]
            if st["bounded"] or y["how"] == "load" or y["uses"] != 1:
                continue
            feat["inplace_forward"] += st["k"] in y["in_roots"]
            hazards += [(a, st["k"], y["how"] != "call") for a in y["in_roots"] if a != st["k"]]
            feat["observed_between"] += st["k"] not in y["in_roots"] and any(
                what == "r" and j == st["k"] and y["pos"] < pos < st["pos"] for what, j, pos in events)
        fn["events"] = events
        fn["features"] = feat
        fn["alias_pair"], fn["alias_write_then_read"], fn["alias_forward_hazard"], fn["alias_runtime_hazard"] = \
            _alias_pair(kinds, events, hazards)
        functions.append(fn)
    head.append("}")
    meta = dict(seed=seed, rank=rank, elem=elem, dtype=np.float64 if elem == "f64" else np.float32, boxes=boxes, ops=ops,
                functions=functions)
    return "\n".join(head) + "\n", meta


def _write_then_read(events, a, b):
    """a store writes argument a (or b) and a kernel reads the other one later"""
    for x, y in ((a, b), (b, a)):
        seen = False
        for what, k, _ in events:
            seen = seen or (what == "w" and k == x)
            if seen and what == "r" and k == y:
                return True
    return False


def _alias_pair(kinds, events, hazards):
    """two same-typed arguments to bind to ONE buffer: the first pair of which one is written and the other read afterwards
    -- of those, first one that is also a forward hazard (a producer reads the one while its result is stored whole into the
    other), and first of all one whose producer is an inline apply or a time_advance, where the runtime's pointer test
    (writes_direct) is all that keeps the kernel out of its input: an opdef checks its destination against its own
    arguments before that -- else a forward hazard, else the first same-typed pair.
    -> ((a, b), whether the write-then-read holds, whether a forward hazard does, whether the runtime-checked one does)"""
    pairs = [(a, b) for a in range(len(kinds)) for b in range(a + 1, len(kinds)) if kinds[a] == kinds[b]]
    wtr = {p: _write_then_read(events, *p) for p in pairs}
    haz = {p: any({a, b} == set(p) for a, b, _ in hazards) for p in pairs}
    hrt = {p: any({a, b} == set(p) and rt for a, b, rt in hazards) for p in pairs}
    best = max(pairs, key=lambda p: (wtr[p] and hrt[p], wtr[p] and haz[p], wtr[p], haz[p]))     # max keeps the first of equals
    return best, wtr[best], haz[best], hrt[best]      # every function has two main-box arguments


def function(meta, name):
    return next(f for f in meta["functions"] if f["name"] == name)


def bindings(meta, fn):
    """the argument bindings to run @fn under: dicts of name, place (one of "d" / "h" per argument) and alias (the pair
    of arguments that are ONE buffer, or None).  The mixed pattern is drawn from the seed, one of each at least."""
    f = function(meta, fn) if isinstance(fn, str) else fn
    n = len(f["kinds"])
    rng = np.random.default_rng([meta["seed"], int(f["name"][2:]), 77])
    place = ["d", "h"] + [str(rng.choice(["d", "h"])) for _ in range(n - 2)]
    place = "".join(place[i] for i in rng.permutation(n))
    return [dict(name="device", place="d" * n, alias=None), dict(name="host", place="h" * n, alias=None),
            dict(name="mixed", place=place, alias=None),
            dict(name="aliased-device", place="d" * n, alias=f["alias_pair"]),
            dict(name="aliased-host", place="h" * n, alias=f["alias_pair"])]


def box_shape(box):
    return tuple(u - l for l, u in zip(*box))


def host_args(meta, fn, binding):
    """fresh numpy arguments of @fn, filled from helpers.hash_field with distinct seeds; the aliased pair is one object"""
    f = function(meta, fn) if isinstance(fn, str) else fn
    args = [helpers.hash_field(box_shape(meta["boxes"][kind]), meta["dtype"], seed=meta["seed"] * 31 + 5 * k + 1)
            for k, kind in enumerate(f["kinds"])]
    if binding["alias"]:
        a, b = binding["alias"]
        args[b] = args[a]
    return args


def oracle_run(module, meta, fn, args):
    """the oracle's @fn on `args` (mutated in place) -> (result, the values a scalar result was summed over, or None)"""
    seen = []
    plain = module._reduce

    def spy(op, src):
        b = op.attrs["bounds"]
        seen.append(np.array(src.data[tuple(slice(l - o, u - o) for l, u, o in zip(b.lb, b.ub, src.lb))]))
        return plain(op, src)
    module._reduce = spy
    try:
        res = module.call(fn, *args)
    finally:
        del module._reduce
    return res, (seen[0] if seen else None)


def reduce_height(meta, f):
    """tree height of the device sum behind @f's scalar result (reduce_cases.tree_height; the operand is a loaded, called
    or time-advanced temp, never a fused apply).  Rank 1-3: the plain reduce over the declared box.  Rank 4: one rank-3
    reduce per leading index (the flat kernel where the box is a whole, aligned sub-buffer, else the box kernel: the
    higher of the two), their results added one by one, and one rounding to the element type."""
    import reduce_cases as rc
    red = f["reduce"]
    box = meta["boxes"][red["kind"]]
    shape = box_shape(box)
    phys = (tuple(l - o for l, o in zip(red["box"][0], box[0])), tuple(u - o for u, o in zip(red["box"][1], box[0])))
    ext = rc.box_ext(shape, phys)
    if meta["rank"] <= 3:
        return rc.tree_height(rc.plain_path(shape, phys), meta["dtype"], ext)
    return max(rc.tree_height(p, meta["dtype"], ext[1:]) for p in ("flat", "box")) + ext[0] + 1


# ---- coverage: what the host test counts over SEEDS ------------------------------------------------------------------
def features(meta, source, report):
    """occurrences per feature in one module: from meta, and from the emitted HIP source / lowering report"""
    c = {}

    def add(key, n=1):
        c[key] = c.get(key, 0) + int(n)
    add(f"rank{meta['rank']}")
    add(meta["elem"])
    names = [f["name"] for f in meta["functions"]]
    for f in meta["functions"]:
        add("result-" + f["result"])
        add("alias-write-then-read", f["alias_write_then_read"])
        add("alias-forward-hazard", f["alias_forward_hazard"])
        add("alias-runtime-hazard", f["alias_runtime_hazard"])
        for k, v in f["features"].items():
            add(k, v)
        body = source.split(f"// ---- @{f['name']} (")[1].split('extern "C"')[0]
        # a producer (an opdef call, an apply, a time_advance) and the destination argument it is given
        dests = re.findall(r"= (?:\w+__impl\(sc|nl::run_\w+<).*?, (&v_\w+|nullptr|dest)(?:, (?:nullptr, nullptr|-?\d+))?\);", body)
        add("forwarded", sum(d.startswith("&v_") for d in dests))
        add("forwarded-apply", len(re.findall(r"= nl::run_\w+<.*, &v_\w+(?:, -?\d+)?\);", body)))
        add("not-forwarded", sum(d == "nullptr" for d in dests))
        add("group-dest-forwarded", len(re.findall(r"const nl::Val\* const dest_\w+\[\] = \{[^}]*&v_", body)))
    for name, _ in meta["ops"]:
        body = source.split(f"// ---- @{name} (")[1].split('extern "C"')[0]
        add("dest-to-returned-producer", len(re.findall(r"nl::run_\w+<.*, dest(?:, -?\d+)?\);", body)))
    add("group", sum(g["function"] in names for g in report["groups"]))
    return c


FLOORS = {k: 2 for k in ("forwarded", "not-forwarded", "dest-to-returned-producer", "group", "load_after_store", "diff_origin",
                         "empty_store", "field_to_field", "second_store", "result-unwrap", "result-temp", "result-scalar",
                         "result-none", "rank1", "rank2", "rank3", "rank4", "f64", "f32", "alias-write-then-read",
                         "time_advance", "inplace_forward", "observed_between",
                         "alias-forward-hazard", "inline_pair", "bounded_store", "full_store",
                         "group-dest-forwarded", "alias-runtime-hazard", "forwarded-apply")}
