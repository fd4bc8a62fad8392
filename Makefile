# Build everything that has to exist before tests / bench run.
#   make            runtime library (HIP, gfx950) + lowering tool + oracle
#   make rt         neptune-pde-solver_amd/lib/libneptune_hip.so
#   make lowering   neptune-pde-solver_amd/bin/neptune-opt + lib/libneptune_lowering.so
#   make oracle     oracle/_build/liboracle.so   (CPU restatement; test infrastructure)
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
CC       ?= gcc
ARCH     ?= gfx950
PKG      := neptune-pde-solver_amd
CSRC     := $(PKG)/csrc
LIBDIR   := $(PKG)/lib
BINDIR   := $(PKG)/bin

# -ffp-contract=off: the reference evaluates stencil bodies op by op, strict IEEE, no FMA
# (lib/Pipeline/NeptuneIRPassesPipeline.cpp:28-46); bit-exact parity needs the same here.
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function \
            -Wno-unused-but-set-variable -Wno-unused-variable
KERNEL_HDRS := $(wildcard $(CSRC)/kernels/*.hpp) $(wildcard $(CSRC)/runtime/*.hpp) include/neptune_hip.h
# names the kernel sources a code object was compiled from: part of every launch-wisdom key (include/neptune_hip.h)
BUILD_ID := $(shell cat $(sort $(KERNEL_HDRS)) | sha256sum | cut -c1-16)
HIPFLAGS += -DNEPTUNE_HIP_BUILD_ID=\"$(BUILD_ID)\"

.PHONY: all rt lowering oracle clean resources
all: rt lowering oracle

# translation units: the runtime proper, one per built-in body (minutes each: every tile of the library -- built side
# by side under make -j), and the host-only slab / wisdom / step-loop / multigrid code (seconds each)
rt: $(LIBDIR)/libneptune_hip.so
build/obj/neptune_hip_rt.o: $(CSRC)/runtime/neptune_hip_rt.hip $(KERNEL_HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
build/obj/rt_body_%.o: $(CSRC)/runtime/rt_body_%.hip $(KERNEL_HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
build/obj/slab_rccl.o: $(CSRC)/runtime/slab_rccl.hip $(KERNEL_HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
build/obj/wisdom.o: $(CSRC)/runtime/wisdom.hip include/neptune_hip.h
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
build/obj/step_loop.o: $(CSRC)/runtime/step_loop.hip $(KERNEL_HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
build/obj/multigrid.o: $(CSRC)/runtime/multigrid.hip $(KERNEL_HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
RT_BODIES := lap2d5 lap3d7 lap3d27 lap1d3
$(LIBDIR)/libneptune_hip.so: build/obj/neptune_hip_rt.o $(RT_BODIES:%=build/obj/rt_body_%.o) build/obj/slab_rccl.o build/obj/wisdom.o build/obj/step_loop.o build/obj/multigrid.o
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared $^ -ldl -o $@

# per-kernel VGPR/SGPR/occupancy table
resources: $(CSRC)/runtime/neptune_hip_rt.hip $(KERNEL_HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c -Rpass-analysis=kernel-resource-usage $< -o build/res.o 2> build/resources.log
	python3 tools/kernel_resources.py build/resources.log

LOWERING_SRCS := $(wildcard $(CSRC)/lowering/*.cpp)
LOWERING_HDRS := $(wildcard $(CSRC)/lowering/*.h)
lowering: $(LIBDIR)/libneptune_lowering.so $(BINDIR)/neptune-opt
$(LIBDIR)/libneptune_lowering.so: $(filter-out %/neptune_opt_main.cpp,$(LOWERING_SRCS)) $(LOWERING_HDRS)
	@mkdir -p $(LIBDIR)
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall $(filter-out %/neptune_opt_main.cpp,$(LOWERING_SRCS)) -o $@
$(BINDIR)/neptune-opt: $(LOWERING_SRCS) $(LOWERING_HDRS)
	@mkdir -p $(BINDIR)
	$(CXX) -O2 -std=c++17 -Wall $(LOWERING_SRCS) -o $@

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIBDIR)/*.so $(BINDIR) oracle/_build
