# Build of the MI355X word-count engine (gfx950).  In-tree outputs so that the
# built .so files travel with the repo snapshot to the GPU box.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-result
# kernels: the scheduler that groups memory instructions into clauses measured
# ~1.5-2 % faster on the C2 bench (k_map 1.16 -> 1.14 ms)
KERNEL_FLAGS ?= -mllvm -amdgpu-sched-strategy=max-memory-clause
PKG := map-oxidize_amd
CSRC := $(PKG)/csrc
OUT := $(PKG)/mox

all: $(OUT)/libmox.so $(OUT)/libmox_corpus.so $(OUT)/meduce-gpu $(OUT)/libmox_check.so $(OUT)/libmox_hc.so oracle

HOST_DEPS := $(CSRC)/mox_host.h $(CSRC)/mox_carve.h $(CSRC)/mox_dev.h $(CSRC)/mox_pack.h $(CSRC)/mox_tiles.h $(CSRC)/mox_wordhash.h $(CSRC)/mox_wordset.h $(CSRC)/mox_internal.h $(CSRC)/mox_table.h include/mox.h

# The calls over the device-resident result, one source each: mox_<op>.hip.
OPS := bsort topk text accum lookup filter rank rekey find hist join
# Those that hash words have a second object in the forced-collision build:
#   accum   the accumulator's packer hashes long words: fnv_finish must truncate there too
#   lookup  the lookup hashes every word it touches: fnv_finish must truncate there too
#   rekey   the re-keying packer hashes long words: fnv_finish must truncate there too
#   join    the join hashes every word of both tables: fnv_finish must truncate there too
# The others hash nothing, so one object serves libmox.so, libmox_check.so and
# libmox_hc.so: the sort, the top-k, the text, the ranking, the search, the
# histograms, and the filter (its list term goes through the _hc lookup).
HC_OPS := accum lookup rekey join

# check build (_check.o, libmox_check.so): device bounds checks on every derived
# index (MOX_CHK, mox_internal.h); tests load it with MOX_LIB=.../libmox_check.so
# forced-collision check build (_hc.o, libmox_hc.so): key hashes truncated to a few
# bits so that every exactness fallback (byte compares behind a hash match) runs,
# with path hit counters and the bounds checks (mox_internal.h, MOX_HASH_COLLIDE);
# tests load it with mox.Engine(lib_path=...) (tests/test_gpu_collide.py)
HC_FLAGS := -DMOX_HASH_COLLIDE -DMOX_CHECK

OP_OBJS := $(OPS:%=$(OUT)/mox_%.o)
OP_HC_OBJS := $(HC_OPS:%=$(OUT)/mox_%_hc.o)
KERNELS_OBJS := $(OUT)/mox_kernels.o $(OUT)/mox_kernels_check.o $(OUT)/mox_kernels_hc.o
# the pass driver and the multi-GPU side hold no kernels; mox_result.hip (the buffer
# helpers of the calls over the result) neither, and it hashes nothing: one object
ENGINE_OBJS := $(OUT)/mox_engine.o $(OUT)/mox_engine_check.o $(OUT)/mox_engine_hc.o
MULTI_OBJS := $(OUT)/mox_multi.o $(OUT)/mox_multi_hc.o

# sources and prerequisites; the objects with kernels also take KERNEL_FLAGS
$(KERNELS_OBJS): $(CSRC)/mox_kernels.hip $(CSRC)/mox_reduce.inc $(CSRC)/mox_internal.h Makefile
$(ENGINE_OBJS): $(CSRC)/mox_engine.hip $(HOST_DEPS) $(CSRC)/mox_unicode_tables.h
$(MULTI_OBJS): $(CSRC)/mox_multi.hip $(HOST_DEPS)
$(OUT)/mox_result.o: $(CSRC)/mox_result.hip $(HOST_DEPS)
$(OP_OBJS): $(OUT)/mox_%.o: $(CSRC)/mox_%.hip $(HOST_DEPS)
$(OP_HC_OBJS): $(OUT)/mox_%_hc.o: $(CSRC)/mox_%.hip $(HOST_DEPS)
$(KERNELS_OBJS) $(OP_OBJS) $(OP_HC_OBJS): KFLAGS := $(KERNEL_FLAGS)

# one rule per variant
$(OUT)/mox_kernels.o $(OUT)/mox_engine.o $(OUT)/mox_multi.o $(OUT)/mox_result.o $(OP_OBJS):
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -c $< -o $@

$(OUT)/mox_kernels_check.o $(OUT)/mox_engine_check.o:
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -DMOX_CHECK -c $< -o $@

$(OUT)/mox_kernels_hc.o $(OUT)/mox_engine_hc.o $(OUT)/mox_multi_hc.o $(OP_HC_OBJS):
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) $(HC_FLAGS) -c $< -o $@

$(OUT)/mox_table.o: $(CSRC)/mox_table.cpp $(CSRC)/mox_table.h
	g++ -O3 -std=c++17 -fPIC -Wall -Wextra -c $< -o $@

# the three libraries: the same objects, each in the library's variant where it has one
COMMON_OBJS := $(OUT)/mox_result.o $(OUT)/mox_table.o
$(OUT)/libmox.so: $(OUT)/mox_kernels.o $(OUT)/mox_engine.o $(OUT)/mox_multi.o $(OP_OBJS) $(COMMON_OBJS)
$(OUT)/libmox_check.so: $(OUT)/mox_kernels_check.o $(OUT)/mox_engine_check.o $(OUT)/mox_multi.o $(OP_OBJS) $(COMMON_OBJS)
$(OUT)/libmox_hc.so: $(OUT)/mox_kernels_hc.o $(OUT)/mox_engine_hc.o $(OUT)/mox_multi_hc.o \
                     $(foreach op,$(OPS),$(OUT)/mox_$(op)$(if $(filter $(op),$(HC_OPS)),_hc).o) $(COMMON_OBJS)
$(OUT)/libmox.so $(OUT)/libmox_check.so $(OUT)/libmox_hc.so:
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

check: $(OUT)/libmox_check.so

hc: $(OUT)/libmox_hc.so

$(OUT)/libmox_corpus.so: $(CSRC)/mox_corpus.c
	gcc -O3 -fPIC -shared -Wall -Wextra -o $@ $< -lpthread -lm

$(OUT)/meduce-gpu: $(CSRC)/meduce_gpu.cpp include/mox.h $(OUT)/libmox.so
	g++ -O2 -std=c++17 -Wall -o $@ $< -Iinclude -L$(OUT) -lmox -Wl,-rpath,'$$ORIGIN'

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(OUT)/*.o $(OUT)/*.so $(OUT)/meduce-gpu
	$(MAKE) -C oracle clean

.PHONY: all clean oracle check hc
