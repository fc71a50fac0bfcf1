# Build the product library (HIP, gfx950) and the CPU oracle (test infrastructure).
HIPCC     ?= /opt/rocm/bin/hipcc
ARCH      ?= gfx950
PKG       := neural_polar_decoder_amd
CSRC      := $(wildcard $(PKG)/csrc/*.hip)
CHDR      := $(wildcard $(PKG)/csrc/*.hpp) include/npd.h
HIPFLAGS  := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Iinclude -I$(PKG)/csrc \
             -munsafe-fp-atomics
LIB       := $(PKG)/libnpd.so
OBJDIR    := build/obj
OBJS      := $(patsubst $(PKG)/csrc/%.hip,$(OBJDIR)/%.o,$(CSRC))

ORACLE    := oracle/liboracle.so

all: $(LIB) $(ORACLE)

lib: $(LIB)
oracle: $(ORACLE)

# per-file extras: the SC and SC-List kernels (npd_sc*) never see NaN (finite LLRs), so fmin needs no canonicalisation
extra = $(if $(filter npd_sc%,$(1)),-fno-honor-nans,$(EXTRA_$(1)))
# the ML/MAP epilogues read every MFMA result on the VALU: keep the accumulators in VGPRs (no v_accvgpr_read per value)
EXTRA_npd_ml := -mllvm -amdgpu-mfma-vgpr-form=1
# the two-tile count sweep uses more than 256 registers; its gate updates read every accumulator on the VALU as well
EXTRA_npd_gru_split16 := -mllvm -amdgpu-mfma-vgpr-form=1

$(OBJDIR)/%.o: $(PKG)/csrc/%.hip $(CHDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(call extra,$*) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -Wl,--no-undefined

# Oracle: plain C, no fast-math, no FMA contraction (exact restatement of the reference's fp32 ops).
# The SCL restatement is C++ so that list pruning calls libstdc++'s std::nth_element (torch.topk's CPU path).
$(ORACLE): oracle/npd_oracle.c oracle/npd_oracle_scl.cpp oracle/npd_oracle_lse.c
	@mkdir -p build/oracle
	gcc -O2 -std=c11 -fPIC -fopenmp -ffp-contract=off -c oracle/npd_oracle.c -o build/oracle/npd_oracle.o
	g++ -O2 -std=c++17 -fPIC -fopenmp -ffp-contract=off -c oracle/npd_oracle_scl.cpp -o build/oracle/npd_oracle_scl.o
	gcc -O2 -std=c11 -fPIC -fopenmp -ffp-contract=off -c oracle/npd_oracle_lse.c -o build/oracle/npd_oracle_lse.o
	g++ -shared -fopenmp -o $@ build/oracle/npd_oracle.o build/oracle/npd_oracle_scl.o build/oracle/npd_oracle_lse.o -lm

asm: $(CSRC)
	@mkdir -p build/asm
	$(foreach b,$(basename $(notdir $(CSRC))),$(HIPCC) $(HIPFLAGS) $(call extra,$(b)) --cuda-device-only -S -o build/asm/$(b).s $(PKG)/csrc/$(b).hip &&) true

clean:
	rm -rf build $(LIB) $(ORACLE)

.PHONY: all lib oracle clean asm
