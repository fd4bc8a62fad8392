"""NeptuneIR text of two-level (leapfrog) steps for tests/test_leapfrog_lowering.py and tests/test_leapfrog_gpu.py:

    u_next = 2 u - u_prev + k * L(u) + 2^-10 * (last index)          k = 1/8, or 1/8 * c with a coefficient field c

as ONE apply of @wave(u, u_prev [, c]) -- `u` read on a star of radius 1 or 2, everything else at the centre -- and
@step(next, cur, prev [, c]) around it.  Every constant is dyadic, so what a literal rounds to cannot differ between the
oracle and the emitted code; the index term makes a shifted logical origin and a wrong plane / row / column visible."""

# star weights per radius: centre (once per dimension), then offsets 1.., all exactly representable in fp32
WEIGHTS = {1: [-2.0, 1.0], 2: [-2.5, 1.25, -0.0625], 3: [-2.5, 1.25, -0.0625, 0.015625]}


def module_text(shape, elem="f64", radius=1, coef=False, origin=None, bounds=None, prev_offset=None):
    """shape: the fields' extent; origin: their logical lower bound (default 0); bounds: the apply's bounds relative to the
    field (default: the box shrunk by the radius); prev_offset: read u_prev at this offset instead of the centre (such a
    body is not a leapfrog candidate)"""
    rank = len(shape)
    lb = list(origin) if origin is not None else [0] * rank
    ub = [l + n for l, n in zip(lb, shape)]
    if bounds is None:
        bounds = ([radius] * rank, [n - radius for n in shape])
    blb = [l + b for l, b in zip(lb, bounds[0])]
    bub = [l + b for l, b in zip(lb, bounds[1])]
    nin = 3 if coef else 2
    dims = "x".join("?" * rank)
    mem = f"memref<{dims}x{elem}>"
    tys = ", ".join(["!t"] * nin)
    names = ["x", "xp", "c"][:nin]
    csv = lambda v: ", ".join(str(x) for x in v)
    L = ['#l = #neptune_ir.location<"cell">',
         f"#b = #neptune_ir.bounds<lb = [{csv(lb)}], ub = [{csv(ub)}]>",
         f"!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>",
         f"!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>",
         "module {",
         f"  neptune_ir.nonlinear_opdef @wave : ({tys}) -> !t {{",
         "  ^bb0(" + ", ".join(f"%u{k}: !t" for k in range(nin)) + "):",
         "    %r = neptune_ir.apply(" + ", ".join(f"%u{k}" for k in range(nin)) + ") attributes {bounds = "
         f"#neptune_ir.bounds<lb = [{csv(blb)}], ub = [{csv(bub)}]>}} : ({tys}) -> !t {{",
         "      ^bb0(" + ", ".join(f"%i{d}: index" for d in range(rank)) + ", " + ", ".join(f"%{n}: !t" for n in names) + "):"]
    W = WEIGHTS[radius]
    zero = [0] * rank
    L += [f"        %x0 = neptune_ir.access %x[{csv(zero)}] : !t -> {elem}",
          f"        %p0 = neptune_ir.access %xp[{csv(prev_offset if prev_offset is not None else zero)}] : !t -> {elem}",
          f"        %w0 = arith.constant {W[0] * rank!r} : {elem}",
          f"        %lap0 = arith.mulf %w0, %x0 : {elem}"]
    lap = "%lap0"
    for s in range(1, radius + 1):
        ring = None
        for d in range(rank):
            for sign in (-1, 1):
                off = list(zero)
                off[d] = sign * s
                v = f"%a{s}_{d}_{'m' if sign < 0 else 'p'}"
                L.append(f"        {v} = neptune_ir.access %x[{csv(off)}] : !t -> {elem}")
                if ring is None:
                    ring = v
                else:
                    nxt = f"%r{s}_{d}_{'m' if sign < 0 else 'p'}"
                    L.append(f"        {nxt} = arith.addf {ring}, {v} : {elem}")
                    ring = nxt
        L += [f"        %w{s} = arith.constant {W[s]!r} : {elem}",
              f"        %t{s} = arith.mulf %w{s}, {ring} : {elem}",
              f"        %lap{s} = arith.addf {lap}, %t{s} : {elem}"]
        lap = f"%lap{s}"
    L += [f"        %two = arith.constant 2.0 : {elem}",
          f"        %k = arith.constant 0.125 : {elem}",
          f"        %d = arith.mulf %two, %x0 : {elem}",
          f"        %e = arith.subf %d, %p0 : {elem}"]
    if coef:
        L += [f"        %c0 = neptune_ir.access %c[{csv(zero)}] : !t -> {elem}",
              f"        %kc = arith.mulf %k, %c0 : {elem}",
              f"        %g = arith.mulf %kc, {lap} : {elem}"]
    else:
        L += [f"        %g = arith.mulf %k, {lap} : {elem}"]
    L += [f"        %h = arith.addf %e, %g : {elem}",
          f"        %iw = arith.index_cast %i{rank - 1} : index to i64",
          f"        %if = arith.sitofp %iw : i64 to {elem}",
          f"        %eps = arith.constant 0.0009765625 : {elem}",
          f"        %ie = arith.mulf %eps, %if : {elem}",
          f"        %o = arith.addf %h, %ie : {elem}",
          f"        neptune_ir.yield %o : {elem}",
          "    }",
          "    neptune_ir.return %r : !t",
          "  }",
          f"  func.func @step(%out: {mem}, " + ", ".join(f"%in{k}: {mem}" for k in range(nin)) + f") -> {mem} {{",
          f"    %fo = neptune_ir.wrap %out : {mem} -> !f"]
    for k in range(nin):
        L += [f"    %f{k} = neptune_ir.wrap %in{k} : {mem} -> !f",
              f"    %t{k} = neptune_ir.load %f{k} : !f -> !t"]
    L += ["    %y = neptune_ir.apply_nonlinear @wave(" + ", ".join(f"%t{k}" for k in range(nin)) + f") : ({tys}) -> !t",
          "    neptune_ir.store %y to %fo : !t to !f",
          f"    %res = neptune_ir.unwrap %fo : !f -> {mem}",
          f"    func.return %res : {mem}",
          "  }", "}"]
    return "\n".join(L) + "\n"


def single_input_text(shape, elem="f64"):
    """the same star on ONE input (a heat-like step): a chain candidate, not a leapfrog one"""
    import test_multihalo_gpu as mh
    rank = len(shape)
    return mh.module_text(shape, elem, 1, [(0, o) for o in mh.star(rank, 1)], [1] * rank, [n - 1 for n in shape])
