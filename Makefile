# Builds the in-tree HIP library for gfx950 (MI355X).  No cmake needed.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := super-resolution-climate_amd
SRC := $(PKG)/csrc
OUT := $(PKG)/srmi/libsrmi.so
OBJDIR ?= build/obj
CXXFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -Iinclude $(EXTRA)
HIPSRC := $(SRC)/conv3x3.hip $(SRC)/conv_f32.hip $(SRC)/wgrad3x3.hip $(SRC)/small.hip $(SRC)/tiles.hip $(SRC)/rcab_infer.hip $(SRC)/spectra.hip $(SRC)/spectral_loss.hip $(SRC)/consistency.hip $(SRC)/ssim.hip $(SRC)/ssim_loss.hip $(SRC)/distribution.hip $(SRC)/quantile_map.hip $(SRC)/gradient.hip $(SRC)/gradient_loss.hip $(SRC)/fss.hip $(SRC)/ensemble_score.hip
CPPSRC := $(SRC)/engine.cpp
OBJS := $(patsubst $(SRC)/%.hip,$(OBJDIR)/%.o,$(HIPSRC)) $(patsubst $(SRC)/%.cpp,$(OBJDIR)/%.o,$(CPPSRC))
HDRS := $(wildcard $(SRC)/*.hpp) include/srmi.h

# the gradient score and loss term state their arithmetic operation by operation (srmi.h): their
# roots and quotients must be the correctly rounded ones, whatever the compiler's default is
GRADOBJS := $(OBJDIR)/gradient.o $(OBJDIR)/gradient_loss.o build/obj_stamps/gradient.o build/obj_stamps/gradient_loss.o
$(GRADOBJS): CXXFLAGS += -fhip-fp32-correctly-rounded-divide-sqrt

# the ensemble score states its fp64 arithmetic operation by operation (srmi.h).  The __d*_rn
# forms are plain operators to this compiler, which fuses a product into a following sum under
# the default contraction setting: the file is built with contraction off
ENSOBJS := $(OBJDIR)/ensemble_score.o build/obj_stamps/ensemble_score.o
$(ENSOBJS): CXXFLAGS += -ffp-contract=off

all: $(OUT)

$(OBJDIR)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(OBJDIR)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(OUT): $(OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(OBJS) -o $@

# diagnostic build with s_memtime phase stamps (tools/kbench.py KBENCH_STAMPS=1)
STAMPOBJDIR := build/obj_stamps
STAMPOUT := $(PKG)/srmi/libsrmi_stamps.so
STAMPOBJS := $(patsubst $(SRC)/%.hip,$(STAMPOBJDIR)/%.o,$(HIPSRC)) $(patsubst $(SRC)/%.cpp,$(STAMPOBJDIR)/%.o,$(CPPSRC))

$(STAMPOBJDIR)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(STAMPOBJDIR)
	$(HIPCC) $(CXXFLAGS) -DSRMI_STAMPS -c $< -o $@

$(STAMPOBJDIR)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(STAMPOBJDIR)
	$(HIPCC) $(CXXFLAGS) -DSRMI_STAMPS -c $< -o $@

$(STAMPOUT): $(STAMPOBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(STAMPOBJS) -o $@

stamps: $(STAMPOUT)

oracle:
	@true

clean:
	rm -rf build $(OUT) $(STAMPOUT)

.PHONY: all clean oracle stamps
