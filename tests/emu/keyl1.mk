# TEST INFRASTRUCTURE ONLY: host builds of the step program with the key
# helper's level-1 key ring (cotix_emu_keyl1.cpp = cotix_emu.cpp + the KeyL1
# help policy) and its stand-alone ASan/UBSan driver.
# make -C tests/emu -f keyl1.mk
CXX ?= g++
FLAGS = -DCOTIX_EMU_POISON -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_emu_keyl1.cpp cotix_emu.cpp cotix_simt.h $(CS)/cotix_kernel.h $(CS)/cotix_plan.h $(CS)/cotix_device.h $(CS)/cotix_scene.h \
	$(CS)/cotix_grad.h $(CS)/cotix_body.h $(CS)/cotix_spec_hdrs.h

all: build/libcotix_emu_keyl1.so build/keyl1_asan_driver

build/libcotix_emu_keyl1.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_emu_keyl1.cpp -o $@

build/keyl1_asan_driver: $(DEPS) keyl1_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_emu_keyl1.cpp keyl1_asan_driver.cpp -o $@
