// RUN: neptune-opt %s --neptuneir-to-hip --report
// Two coupled 3-D fields (u, v), 512^3 f64, advanced by two sibling applies of 7-point shape over the same two inputs:
//   u' = u + dt (k lap7(u) - v),   v' = v + dt (k lap7(v) + u)
// Member 0 lists u first, member 1 lists v first (input 0: result type and copy-through source).  Authored for this
// backend: the smallest 3-D system the multi-output launch applies to -- two results for one read of each input.
// Only IEEE-exact operations, evaluated in textual order.

#loc = #neptune_ir.location<"cell">
#b   = #neptune_ir.bounds<lb = [0, 0, 0], ub = [512, 512, 512]>
#bi  = #neptune_ir.bounds<lb = [1, 1, 1], ub = [511, 511, 511]>

!temp  = !neptune_ir.temp<element = f64, bounds = #b, location = #loc>
!field = !neptune_ir.field<element = f64, bounds = #b, location = #loc>

module {
  func.func @entry(%ou: memref<?x?x?xf64>, %ov: memref<?x?x?xf64>, %iu: memref<?x?x?xf64>, %iv: memref<?x?x?xf64>)
      -> memref<?x?x?xf64> {
    %fou = neptune_ir.wrap %ou : memref<?x?x?xf64> -> !field
    %fov = neptune_ir.wrap %ov : memref<?x?x?xf64> -> !field
    %fu  = neptune_ir.wrap %iu : memref<?x?x?xf64> -> !field
    %fv  = neptune_ir.wrap %iv : memref<?x?x?xf64> -> !field
    %u   = neptune_ir.load %fu : !field -> !temp
    %v   = neptune_ir.load %fv : !field -> !temp
    %ru = neptune_ir.apply(%u, %v) attributes {bounds = #bi} : (!temp, !temp) -> !temp {
      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp):
        %c  = neptune_ir.access %a[0, 0, 0] : !temp -> f64
        %xm = neptune_ir.access %a[-1, 0, 0] : !temp -> f64
        %xp = neptune_ir.access %a[1, 0, 0] : !temp -> f64
        %ym = neptune_ir.access %a[0, -1, 0] : !temp -> f64
        %yp = neptune_ir.access %a[0, 1, 0] : !temp -> f64
        %zm = neptune_ir.access %a[0, 0, -1] : !temp -> f64
        %zp = neptune_ir.access %a[0, 0, 1] : !temp -> f64
        %w  = neptune_ir.access %o[0, 0, 0] : !temp -> f64
        %six = arith.constant 6.0 : f64
        %k   = arith.constant 0.0625 : f64
        %dt  = arith.constant 0.25 : f64
        %t0  = arith.addf %xm, %xp : f64
        %t1  = arith.addf %t0, %ym : f64
        %t2  = arith.addf %t1, %yp : f64
        %t3  = arith.addf %t2, %zm : f64
        %t4  = arith.addf %t3, %zp : f64
        %t5  = arith.mulf %six, %c : f64
        %t6  = arith.subf %t4, %t5 : f64
        %lap = arith.mulf %k, %t6 : f64
        %rhs = arith.subf %lap, %w : f64
        %inc = arith.mulf %dt, %rhs : f64
        %r   = arith.addf %c, %inc : f64
        neptune_ir.yield %r : f64
      }
    %rv = neptune_ir.apply(%v, %u) attributes {bounds = #bi} : (!temp, !temp) -> !temp {
      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp):
        %c  = neptune_ir.access %a[0, 0, 0] : !temp -> f64
        %xm = neptune_ir.access %a[-1, 0, 0] : !temp -> f64
        %xp = neptune_ir.access %a[1, 0, 0] : !temp -> f64
        %ym = neptune_ir.access %a[0, -1, 0] : !temp -> f64
        %yp = neptune_ir.access %a[0, 1, 0] : !temp -> f64
        %zm = neptune_ir.access %a[0, 0, -1] : !temp -> f64
        %zp = neptune_ir.access %a[0, 0, 1] : !temp -> f64
        %w  = neptune_ir.access %o[0, 0, 0] : !temp -> f64
        %six = arith.constant 6.0 : f64
        %k   = arith.constant 0.0625 : f64
        %dt  = arith.constant 0.25 : f64
        %t0  = arith.addf %xm, %xp : f64
        %t1  = arith.addf %t0, %ym : f64
        %t2  = arith.addf %t1, %yp : f64
        %t3  = arith.addf %t2, %zm : f64
        %t4  = arith.addf %t3, %zp : f64
        %t5  = arith.mulf %six, %c : f64
        %t6  = arith.subf %t4, %t5 : f64
        %lap = arith.mulf %k, %t6 : f64
        %rhs = arith.addf %lap, %w : f64
        %inc = arith.mulf %dt, %rhs : f64
        %r   = arith.addf %c, %inc : f64
        neptune_ir.yield %r : f64
      }
    neptune_ir.store %ru to %fou : !temp to !field
    neptune_ir.store %rv to %fov : !temp to !field
    %res = neptune_ir.unwrap %fou : !field -> memref<?x?x?xf64>
    func.return %res : memref<?x?x?xf64>
  }
}
