#!/usr/bin/env python3
"""Matrix-free conjugate gradients on device-resident vectors, with the operator and the dot products
lowered from NeptuneIR: what the reference does through PETSc's MatShell +
KSP on the host (lib/Runtime/PETSc/NeptunePETScRuntime.cpp:182-230, 719-786), without leaving the GPU.

    A    : linear_opdef, 7-point negative Laplacian on the interior, identity on the rim (copy-through)
    dot  : reduce(apply(a*b)) -- one fused kernel, reads both vectors once
    axpy : plain torch (NeptuneIR regions are IsolatedFromAbove: a run-time scalar cannot enter an apply)

With --solver the same problem runs through neptune_hip.apply.cg_solve instead: the loop, its scalars and its
vector updates stay on the device, p . A(p) comes out of the launch that computes A(p) (lowering option dot-entries), and the
host reads one scalar every 10 iterations.

usage: examples/cg_matrix_free.py [N] [--solver]      (default 256: a 256^3 Poisson problem)"""
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))


def module_text(shape):
    n0, n1, n2 = shape
    return f"""
#l = #neptune_ir.location<"cell">
#b = #neptune_ir.bounds<lb = [0, 0, 0], ub = [{n0}, {n1}, {n2}]>
!t = !neptune_ir.temp<element = f64, bounds = #b, location = #l>
!f = !neptune_ir.field<element = f64, bounds = #b, location = #l>
module {{
  neptune_ir.linear_opdef @A : (!t) -> !t {{
  ^bb0(%u: !t):
    %r = neptune_ir.apply(%u) attributes {{bounds = #neptune_ir.bounds<lb = [1, 1, 1], ub = [{n0 - 1}, {n1 - 1}, {n2 - 1}]>}} : (!t) -> !t {{
      ^bb0(%i: index, %j: index, %k: index, %a: !t):
        %c = neptune_ir.access %a[0, 0, 0] : !t -> f64
        %xm = neptune_ir.access %a[-1, 0, 0] : !t -> f64
        %xp = neptune_ir.access %a[1, 0, 0] : !t -> f64
        %ym = neptune_ir.access %a[0, -1, 0] : !t -> f64
        %yp = neptune_ir.access %a[0, 1, 0] : !t -> f64
        %zm = neptune_ir.access %a[0, 0, -1] : !t -> f64
        %zp = neptune_ir.access %a[0, 0, 1] : !t -> f64
        %six = arith.constant 6.0 : f64
        %t0 = arith.addf %xm, %xp : f64
        %t1 = arith.addf %t0, %ym : f64
        %t2 = arith.addf %t1, %yp : f64
        %t3 = arith.addf %t2, %zm : f64
        %t4 = arith.addf %t3, %zp : f64
        %t5 = arith.mulf %six, %c : f64
        %t6 = arith.subf %t5, %t4 : f64
        neptune_ir.yield %t6 : f64
    }}
    neptune_ir.return %r : !t
  }}
  func.func @matmult(%y: memref<?x?x?xf64>, %x: memref<?x?x?xf64>) -> memref<?x?x?xf64> {{
    %fy = neptune_ir.wrap %y : memref<?x?x?xf64> -> !f
    %fx = neptune_ir.wrap %x : memref<?x?x?xf64> -> !f
    %u = neptune_ir.load %fx : !f -> !t
    %v = neptune_ir.apply_linear @A(%u) : (!t) -> !t
    neptune_ir.store %v to %fy : !t to !f
    %res = neptune_ir.unwrap %fy : !f -> memref<?x?x?xf64>
    func.return %res : memref<?x?x?xf64>
  }}
  func.func @dot(%a: memref<?x?x?xf64>, %b: memref<?x?x?xf64>) -> f64 {{
    %fa = neptune_ir.wrap %a : memref<?x?x?xf64> -> !f
    %fb = neptune_ir.wrap %b : memref<?x?x?xf64> -> !f
    %u = neptune_ir.load %fa : !f -> !t
    %v = neptune_ir.load %fb : !f -> !t
    %w = neptune_ir.apply(%u, %v) attributes {{bounds = #b}} : (!t, !t) -> !t {{
      ^bb0(%i: index, %j: index, %k: index, %p: !t, %q: !t):
        %x = neptune_ir.access %p[0, 0, 0] : !t -> f64
        %y = neptune_ir.access %q[0, 0, 0] : !t -> f64
        %m = arith.mulf %x, %y : f64
        neptune_ir.yield %m : f64
    }}
    %s = neptune_ir.reduce %w {{kind = "sum"}} : !t -> f64
    func.return %s : f64
  }}
}}
"""


def cg(matmult, dot, b, x, tol=1e-10, maxit=500):
    """textbook CG; vectors are whatever `matmult`/`dot` accept (torch CUDA tensors or numpy arrays)"""
    r = b.clone() if hasattr(b, "clone") else b.copy()
    ap = r * 0
    matmult(ap, x)
    r -= ap
    p = r.clone() if hasattr(r, "clone") else r.copy()
    rs = dot(r, r)
    rs0 = rs
    it = 0
    while it < maxit and rs > tol * tol * rs0:
        matmult(ap, p)
        alpha = rs / dot(p, ap)
        x += alpha * p
        r -= alpha * ap
        rs_new = dot(r, r)
        p *= rs_new / rs
        p += r
        rs = rs_new
        it += 1
    return x, it, (rs / rs0) ** 0.5


def run_solver(shape, b, tol):
    """the same solve through neptune_hip_cg_solve: -> (iterations, relative residual, seconds)"""
    import torch
    from neptune_hip import _capi, apply, fields, lowering
    mod = lowering.compile_module(module_text(shape), dot_entries=True)
    entry = mod.dot_entry(next(a["function"] for a in mod.report["applies"] if a.get("dot_symbol")))
    interior = ([1, 1, 1], [n - 1 for n in shape])
    field = lambda t: fields.DeviceField((0, 0, 0), shape, _capi.F64, t)
    work = [field(torch.empty_like(b)) for _ in range(3)]
    _, rr0, _ = apply.cg_solve(entry, field(torch.zeros_like(b)), field(b), interior, 0, 0.0, work=work)   # r . r of the first guess
    x = field(torch.zeros_like(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it, _, rr = apply.cg_solve(entry, x, field(b), interior, 500, tol * tol * rr0, check_every=10, work=work)
    return it, (rr / rr0) ** 0.5, time.perf_counter() - t0


def main():
    args = [a for a in sys.argv[1:] if a != "--solver"]
    n = int(args[0]) if args else 256
    import torch
    from neptune_hip import lowering
    shape = (n, n, n)
    mod = lowering.compile_module(module_text(shape))
    print("kernels:", [(a["function"], a["kernel"]) for a in mod.report["applies"]])
    g = torch.Generator(device="cuda").manual_seed(7)
    b = torch.zeros(shape, dtype=torch.float64, device="cuda")
    b[1:-1, 1:-1, 1:-1] = torch.rand((n - 2,) * 3, dtype=torch.float64, device="cuda", generator=g)
    if "--solver" in sys.argv[1:]:
        it, rel, dt = run_solver(shape, b, 1e-8)
        print(f"{n}^3 Poisson, cg_solve: {it} iterations, relative residual {rel:.2e}, {dt * 1e3 / max(it, 1):.3f} ms per iteration")
        return
    x = torch.zeros_like(b)
    t0 = time.perf_counter()
    x, it, rel = cg(lambda y, v: mod.call("matmult", y, v), lambda u, v: mod.call("dot", u, v), b, x, tol=1e-8)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{n}^3 Poisson, CG: {it} iterations, relative residual {rel:.2e}, {dt * 1e3 / max(it, 1):.3f} ms per iteration")


if __name__ == "__main__":
    main()
