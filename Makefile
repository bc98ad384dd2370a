# Build libpaoship.so (gfx950) and the CPU-side helpers.  `python -c "import __graft_entry__ as g; g.build()"`
# runs the same commands with the same flags.
HIPCC ?= hipcc
ARCH ?= gfx950
# EXTRA: experiment flags for every HIP translation unit of the library, e.g. make EXTRA=-DPAOS_BR=8
HIPFLAGS = -O3 --offload-arch=$(ARCH) -ffp-contract=off -fPIC -std=c++17 -Wall $(EXTRA)
CSRC = paos_amd/csrc
LIB = paos_amd/libpaoship.so

all: $(LIB)

# The library is every csrc/*.hip (one object each, all compiled alike: make -j) and every csrc/*.cpp (host code).
# Every object depends on every header, and so does the hash of what the library was built from.
HIP_SRCS = $(sort $(wildcard $(CSRC)/*.hip))
CPP_SRCS = $(sort $(wildcard $(CSRC)/*.cpp))
HEADERS = $(sort $(wildcard $(CSRC)/*.h include/*.h))
HIP_OBJS = $(patsubst $(CSRC)/%.hip,build/obj/hip/%.o,$(HIP_SRCS))
OBJS = $(HIP_OBJS) $(patsubst $(CSRC)/%.cpp,build/obj/%.o,$(CPP_SRCS)) build/obj/srchash.o

# What the library was built from: __graft_entry__.source_hash() over the sources and headers above (paos_source_hash();
# build() compares it with the tree and rebuilds on a mismatch -- a prebuilt .so that travelled with the tree cannot
# silently be stale)
build/obj/srchash.o: $(HIP_SRCS) $(CPP_SRCS) $(HEADERS) __graft_entry__.py
	mkdir -p build/obj
	printf 'extern "C" const char* paos_source_hash(void) { return "%s"; }\n' "$$(python3 -c 'import __graft_entry__ as g; print(g.source_hash())')" > build/obj/srchash.cpp
	g++ -O2 -fPIC -c build/obj/srchash.cpp -o $@

build/obj/hip/%.o: $(CSRC)/%.hip $(HEADERS)
	mkdir -p build/obj/hip
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -c $< -o $@

# host code only, e.g. the multi-GPU fan-out (include/paos_comm.h; RCCL is dlopen'ed at run time) ...
build/obj/%.o: $(CSRC)/%.cpp $(HEADERS)
	mkdir -p build/obj
	$(HIPCC) -O2 -fPIC -std=c++17 -Wall -c $< -o $@

# ... except the scalar half of the propagation loop for a batch (include/paos_plan.h): plain C++ by the host compiler, the
# reference's operation order, no FMA contraction
build/obj/paos_plan.o: $(CSRC)/paos_plan.cpp $(HEADERS)
	mkdir -p build/obj
	g++ -O2 -fPIC -std=c++17 -Wall -ffp-contract=off -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) -shared -fPIC $(OBJS) -ldl -o $(LIB)

build/fftbench: tools/fftbench.hip $(HEADERS)
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -ffp-contract=off -I$(CSRC) tools/fftbench.hip -o build/fftbench

# every pass-kernel shape should fit its register budget without scratch: rebuild with the compiler's resource remarks
# and list the shapes that spill (a change that costs a shape its allocation shows here, not only in the bench).
# --output-sync: the report reads whole blocks of remarks, which the compilers of a parallel build would interleave
spillcheck:
	mkdir -p build
	$(MAKE) -B -j6 --output-sync=target EXTRA=-Rpass-analysis=kernel-resource-usage > build/make.log 2>&1
	python3 tools/spill_report.py build/make.log

clean:
	rm -f $(LIB) $(OBJS) build/fftbench
