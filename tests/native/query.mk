# TEST INFRASTRUCTURE: helpers for tests/test_ray_query.py (built by __graft_entry__.build() and, when
# missing, by the test module itself):  make -C tests/native -f query.mk
HIPCC ?= /opt/rocm/bin/hipcc
PKG   := ../../ray-tracing-c_amd
all: bin/libray_query_ref.so bin/query_host_check
.PHONY: all
# the ray-query checker: the oracle's hit methods over a batch of rays
bin/libray_query_ref.so: ray_query_ref.c ../../oracle/oracle.c $(wildcard ../../include/*.h)
	@mkdir -p bin
	gcc -std=c11 -O2 -ffp-contract=off -fPIC -shared -I../../include -o $@ ray_query_ref.c -lm
# the ray-query kernel's per-lane code and refill rounds (rt_query.h) on the host, AddressSanitizer on the
# host side (no GPU sanitizer), as kernel_host_check is built
bin/query_host_check: query_host_check.cpp $(PKG)/csrc/rt_query.h $(PKG)/csrc/rt_device.h $(PKG)/csrc/rt_libm.h $(PKG)/librtc_amd.so
	@mkdir -p bin
	$(HIPCC) -x hip --offload-arch=gfx950 --offload-host-only -O1 -g -ffp-contract=off -fno-fast-math \
	    -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -std=c++17 \
	    query_host_check.cpp -o $@ -L$(PKG) -lrtc_amd -Wl,-rpath,'$$ORIGIN/../../../ray-tracing-c_amd' -lm
