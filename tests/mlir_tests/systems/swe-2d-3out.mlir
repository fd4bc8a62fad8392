// RUN: neptune-opt %s --neptuneir-to-hip --report
// 2-D shallow-water step on (h, qx, qy), 8192^2 f64: one residual-style update per unknown, written as three sibling
// applies over the same three fields.  Each member lists ITS unknown first (input 0: result type and copy-through
// source outside apply.bounds); together they read all three fields at +-1 along both dimensions, and the momentum
// updates divide by h.  Authored for this backend: a SYSTEM of equations as the lowering sees it -- consecutive applies
// with shared operands, each stored to its own field -- which one multi-output launch computes in a single pass.
//   h'  = h  - a ((qx[+1,0] - qx[-1,0]) + (qy[0,+1] - qy[0,-1])) + nu (h[-1,0] + h[+1,0] + h[0,-1] + h[0,+1] - 4 h)
//   qx' = qx - a ((F[+1,0] - F[-1,0]) + (G[0,+1] - G[0,-1])),  F = qx qx / h + g2 h h,  G = qx qy / h
//   qy' = qy - a ((G'[+1,0] - G'[-1,0]) + (F'[0,+1] - F'[0,-1])),  G' = qy qx / h,  F' = qy qy / h + g2 h h
// Only IEEE-exact operations (add, sub, mul, div), evaluated in textual order.

#loc = #neptune_ir.location<"cell">
#b   = #neptune_ir.bounds<lb = [0, 0], ub = [8192, 8192]>
#bi  = #neptune_ir.bounds<lb = [1, 1], ub = [8191, 8191]>

!temp  = !neptune_ir.temp<element = f64, bounds = #b, location = #loc>
!field = !neptune_ir.field<element = f64, bounds = #b, location = #loc>

module {
  func.func @entry(%oh: memref<?x?xf64>, %oqx: memref<?x?xf64>, %oqy: memref<?x?xf64>,
                   %ih: memref<?x?xf64>, %iqx: memref<?x?xf64>, %iqy: memref<?x?xf64>) -> memref<?x?xf64> {
    %foh  = neptune_ir.wrap %oh  : memref<?x?xf64> -> !field
    %foqx = neptune_ir.wrap %oqx : memref<?x?xf64> -> !field
    %foqy = neptune_ir.wrap %oqy : memref<?x?xf64> -> !field
    %fh   = neptune_ir.wrap %ih  : memref<?x?xf64> -> !field
    %fqx  = neptune_ir.wrap %iqx : memref<?x?xf64> -> !field
    %fqy  = neptune_ir.wrap %iqy : memref<?x?xf64> -> !field
    %h    = neptune_ir.load %fh  : !field -> !temp
    %qx   = neptune_ir.load %fqx : !field -> !temp
    %qy   = neptune_ir.load %fqy : !field -> !temp
    %rh = neptune_ir.apply(%h, %qx, %qy) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {
      ^bb0(%i: index, %j: index, %ah: !temp, %ax: !temp, %ay: !temp):
        %hc = neptune_ir.access %ah[0, 0] : !temp -> f64
        %hw = neptune_ir.access %ah[-1, 0] : !temp -> f64
        %he = neptune_ir.access %ah[1, 0] : !temp -> f64
        %hs = neptune_ir.access %ah[0, -1] : !temp -> f64
        %hn = neptune_ir.access %ah[0, 1] : !temp -> f64
        %xw = neptune_ir.access %ax[-1, 0] : !temp -> f64
        %xe = neptune_ir.access %ax[1, 0] : !temp -> f64
        %ys = neptune_ir.access %ay[0, -1] : !temp -> f64
        %yn = neptune_ir.access %ay[0, 1] : !temp -> f64
        %a    = arith.constant 0.125 : f64
        %nu   = arith.constant 0.03125 : f64
        %four = arith.constant 4.0 : f64
        %dx   = arith.subf %xe, %xw : f64
        %dy   = arith.subf %yn, %ys : f64
        %div  = arith.addf %dx, %dy : f64
        %adv  = arith.mulf %a, %div : f64
        %s0   = arith.addf %hw, %he : f64
        %s1   = arith.addf %s0, %hs : f64
        %s2   = arith.addf %s1, %hn : f64
        %c4   = arith.mulf %four, %hc : f64
        %lap  = arith.subf %s2, %c4 : f64
        %dif  = arith.mulf %nu, %lap : f64
        %t0   = arith.subf %hc, %adv : f64
        %r    = arith.addf %t0, %dif : f64
        neptune_ir.yield %r : f64
      }
    %rqx = neptune_ir.apply(%qx, %h, %qy) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {
      ^bb0(%i: index, %j: index, %am: !temp, %ah: !temp, %ao: !temp):
        %mc = neptune_ir.access %am[0, 0] : !temp -> f64
        %mm = neptune_ir.access %am[-1, 0] : !temp -> f64
        %mp = neptune_ir.access %am[1, 0] : !temp -> f64
        %nm = neptune_ir.access %am[0, -1] : !temp -> f64
        %np = neptune_ir.access %am[0, 1] : !temp -> f64
        %hm = neptune_ir.access %ah[-1, 0] : !temp -> f64
        %hp = neptune_ir.access %ah[1, 0] : !temp -> f64
        %km = neptune_ir.access %ah[0, -1] : !temp -> f64
        %kp = neptune_ir.access %ah[0, 1] : !temp -> f64
        %om = neptune_ir.access %ao[0, -1] : !temp -> f64
        %op = neptune_ir.access %ao[0, 1] : !temp -> f64
        %a    = arith.constant 0.125 : f64
        %g2   = arith.constant 0.5 : f64
        %up   = arith.divf %mp, %hp : f64
        %fp0  = arith.mulf %mp, %up : f64
        %pp0  = arith.mulf %hp, %hp : f64
        %pp   = arith.mulf %g2, %pp0 : f64
        %fp   = arith.addf %fp0, %pp : f64
        %um   = arith.divf %mm, %hm : f64
        %fm0  = arith.mulf %mm, %um : f64
        %pm0  = arith.mulf %hm, %hm : f64
        %pm   = arith.mulf %g2, %pm0 : f64
        %fm   = arith.addf %fm0, %pm : f64
        %vp   = arith.divf %op, %kp : f64
        %gp   = arith.mulf %np, %vp : f64
        %vm   = arith.divf %om, %km : f64
        %gm   = arith.mulf %nm, %vm : f64
        %df   = arith.subf %fp, %fm : f64
        %dg   = arith.subf %gp, %gm : f64
        %sum  = arith.addf %df, %dg : f64
        %adv  = arith.mulf %a, %sum : f64
        %r    = arith.subf %mc, %adv : f64
        neptune_ir.yield %r : f64
      }
    %rqy = neptune_ir.apply(%qy, %h, %qx) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {
      ^bb0(%i: index, %j: index, %am: !temp, %ah: !temp, %ao: !temp):
        %mc = neptune_ir.access %am[0, 0] : !temp -> f64
        %mm = neptune_ir.access %am[0, -1] : !temp -> f64
        %mp = neptune_ir.access %am[0, 1] : !temp -> f64
        %nm = neptune_ir.access %am[-1, 0] : !temp -> f64
        %np = neptune_ir.access %am[1, 0] : !temp -> f64
        %hm = neptune_ir.access %ah[0, -1] : !temp -> f64
        %hp = neptune_ir.access %ah[0, 1] : !temp -> f64
        %km = neptune_ir.access %ah[-1, 0] : !temp -> f64
        %kp = neptune_ir.access %ah[1, 0] : !temp -> f64
        %om = neptune_ir.access %ao[-1, 0] : !temp -> f64
        %op = neptune_ir.access %ao[1, 0] : !temp -> f64
        %a    = arith.constant 0.125 : f64
        %g2   = arith.constant 0.5 : f64
        %up   = arith.divf %mp, %hp : f64
        %fp0  = arith.mulf %mp, %up : f64
        %pp0  = arith.mulf %hp, %hp : f64
        %pp   = arith.mulf %g2, %pp0 : f64
        %fp   = arith.addf %fp0, %pp : f64
        %um   = arith.divf %mm, %hm : f64
        %fm0  = arith.mulf %mm, %um : f64
        %pm0  = arith.mulf %hm, %hm : f64
        %pm   = arith.mulf %g2, %pm0 : f64
        %fm   = arith.addf %fm0, %pm : f64
        %vp   = arith.divf %op, %kp : f64
        %gp   = arith.mulf %np, %vp : f64
        %vm   = arith.divf %om, %km : f64
        %gm   = arith.mulf %nm, %vm : f64
        %df   = arith.subf %fp, %fm : f64
        %dg   = arith.subf %gp, %gm : f64
        %sum  = arith.addf %df, %dg : f64
        %adv  = arith.mulf %a, %sum : f64
        %r    = arith.subf %mc, %adv : f64
        neptune_ir.yield %r : f64
      }
    neptune_ir.store %rh  to %foh  : !temp to !field
    neptune_ir.store %rqx to %foqx : !temp to !field
    neptune_ir.store %rqy to %foqy : !temp to !field
    %res = neptune_ir.unwrap %foh : !field -> memref<?x?xf64>
    func.return %res : memref<?x?xf64>
  }
}
