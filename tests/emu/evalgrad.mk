# TEST INFRASTRUCTURE ONLY: host builds of the differentiable eval
# (cotix_emu_evalgrad.cpp = cotix_emu.cpp + the saving eval forward and its
# tape backward): the plain library, phase G's tile form on every scene
# (-DCOTIX_NO_GREGS), and the stand-alone ASan/UBSan driver.
# make -C tests/emu -f evalgrad.mk
CXX ?= g++
FLAGS = -DCOTIX_EMU_POISON -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_emu_evalgrad.cpp cotix_emu.cpp cotix_simt.h $(CS)/cotix_kernel.h $(CS)/cotix_plan.h $(CS)/cotix_device.h $(CS)/cotix_scene.h \
	$(CS)/cotix_grad.h $(CS)/cotix_body.h $(CS)/cotix_spec_hdrs.h

all: build/libcotix_emu_evalgrad.so build/libcotix_emu_evalgrad_nogregs.so build/evalgrad_asan_driver

build/libcotix_emu_evalgrad.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_emu_evalgrad.cpp -o $@

build/libcotix_emu_evalgrad_nogregs.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -DCOTIX_NO_GREGS -fPIC -shared cotix_emu_evalgrad.cpp -o $@

build/evalgrad_asan_driver: $(DEPS) evalgrad_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_emu_evalgrad.cpp evalgrad_asan_driver.cpp -o $@
