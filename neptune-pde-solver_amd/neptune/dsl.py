"""DSL decorators and top-level instructions (mirror of python_frontend/neptune/dsl.py:5-74)."""
from .core import get_compiler
from .expr import Expr


def apply(inputs, bounds, through=None):
    """@neptune.apply(inputs=[u, v], bounds=([1], [9]))
    def kernel(u, v): ...        -> Expr wrapping the apply's result temp

    A kernel that returns a tuple or list of Exprs (a system: `return res_h, res_q`) creates one apply per element, all
    over the same inputs and bounds, in order, and the decorator returns a tuple of result Exprs.  The function is traced
    once per element and each region keeps only what its own value needs.  `through=(i0, i1, ...)` names, per element,
    which input is that apply's input 0 -- its copy-through source outside `bounds` and its result type; the function
    still receives its arguments in the declared order.  Default: input 0 for every element.  The HIP lowering runs such
    sibling applies as one multi-output kernel where it can."""
    lb, ub = bounds
    compiler = get_compiler()
    handles = [i._handle for i in inputs]

    def decorator(func):
        state = {"count": None}

        def order(first):          # the apply's operand order when declared input `first` is its input 0
            return [first] + [k for k in range(len(handles)) if k != first]

        def member(m, first):
            perm = order(first)

            def body(arg_handles):
                declared = [None] * len(perm)
                for pos, k in enumerate(perm):
                    declared[k] = Expr(arg_handles[pos])
                result = func(*declared)
                if isinstance(result, Expr):
                    if m != 0 or through is not None:
                        raise TypeError("Kernel returned a single Expr where a tuple was expected")
                    return result._handle
                if not isinstance(result, (tuple, list)) or not result or not all(isinstance(r, Expr) for r in result):
                    raise TypeError(f"Kernel must return a Neptune Expr, got {type(result)}")
                if state["count"] is None:
                    state["count"] = len(result)
                elif state["count"] != len(result):
                    raise TypeError("Kernel returned a different number of values when traced again")
                return result[m]._handle

            # a single Expr keeps the region exactly as traced; a member of a tuple drops the other members' ops
            return Expr(compiler.create_apply([handles[k] for k in perm], lb, ub, body, prune=lambda: state["count"] is not None))

        if through is not None and any(not 0 <= int(t) < len(handles) for t in through):
            raise ValueError("through: input index out of range")
        first = member(0, int(through[0]) if through is not None else 0)
        if state["count"] is None:
            return first
        if through is not None and len(through) != state["count"]:
            raise ValueError(f"through names {len(through)} inputs for a kernel that returns {state['count']} values")
        return (first,) + tuple(member(m, int(through[m]) if through is not None else 0) for m in range(1, state["count"]))

    return decorator


stencil = apply


def linear_op_def(bounds, location, name=None, apply_bounds=None):
    """Define a linear operator symbol; the scalar kernel is wrapped in one neptune_ir.apply.

    `apply_bounds` (extension) restricts the apply to a sub-box, typically the interior, so that
    neighbour accesses stay inside the field; the reference applies the kernel over the whole box
    (dsl.py:41-45), which reads out of bounds for any stencil with a non-zero offset."""
    compiler = get_compiler()

    def decorator(func):
        symbol_name = name if name else func.__name__
        lb, ub = apply_bounds if apply_bounds is not None else bounds

        def op_def_body(op_args):
            def apply_body(apply_args):
                return func(*[Expr(h) for h in apply_args])._handle

            return compiler.create_apply(op_args, lb, ub, apply_body)

        compiler.create_linear_opdef(symbol_name, bounds[0], bounds[1], location, op_def_body)
        return symbol_name

    return decorator


def assemble_matrix(op_symbol_name):
    """H = neptune.assemble_matrix("laplacian")   (solver surface: host PETSc path)"""
    return Expr(get_compiler().create_assemble_matrix(op_symbol_name))


def solve_linear(matrix, rhs, solver="cg", tol=1e-6):
    return Expr(get_compiler().create_solve_linear(matrix._handle, rhs._handle, solver, tol))
