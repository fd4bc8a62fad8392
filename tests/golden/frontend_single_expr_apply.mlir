module {
  func.func @blend(%arg0: memref<?x?xf64>, %arg1: memref<?x?xf64>, %arg2: memref<?x?xf64>) -> memref<?x?xf64> {
    %f1 = neptune_ir.wrap %arg0 : memref<?x?xf64> -> !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %f2 = neptune_ir.wrap %arg1 : memref<?x?xf64> -> !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %t3 = neptune_ir.load %f2 : !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %f4 = neptune_ir.wrap %arg2 : memref<?x?xf64> -> !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %t5 = neptune_ir.load %f4 : !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %r6 = neptune_ir.apply(%t3, %t5) attributes {bounds = #neptune_ir.bounds<lb = [1, 1], ub = [9, 15]>}
      : (!neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>, !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>) -> !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> {
    ^bb0(%i7: index, %i8: index, %in9: !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>, %in10: !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>):
      %a11 = neptune_ir.access %in10[0, 1] : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> f64
      %c12 = arith.constant 3.0 : f64
      %v13 = arith.mulf %a11, %c12 : f64
      %a14 = neptune_ir.access %in9[-1, 0] : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> f64
      %a15 = neptune_ir.access %in9[1, 0] : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> f64
      %v16 = arith.addf %a14, %a15 : f64
      %c17 = arith.constant 0.5 : f64
      %v18 = arith.mulf %v16, %c17 : f64
      %a19 = neptune_ir.access %in10[0, 0] : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> f64
      %a20 = neptune_ir.access %in9[0, 0] : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> f64
      %c21 = arith.constant 2.0 : f64
      %v22 = arith.addf %a20, %c21 : f64
      %v23 = arith.divf %a19, %v22 : f64
      %v24 = arith.subf %v18, %v23 : f64
      neptune_ir.yield %v24 : f64
    }
    neptune_ir.store %r6 to %f1 : !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> to !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">>
    %m25 = neptune_ir.unwrap %f1 : !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0], ub = [10, 16]>, location = #neptune_ir.location<"cell">> -> memref<?x?xf64>
    func.return %m25 : memref<?x?xf64>
  }
}
