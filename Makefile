# Build everything in-tree.  `make` = host library + HIP library + CLI; `make oracle` = the test checker.
ROCM    ?= /opt/rocm
HIPCC   ?= $(ROCM)/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -fPIC -Iinclude
HIPFLAGS = -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Iinclude -Wall -Wno-unused-result

LIBDIR = seeksv_amd/lib
HOST_SRC = seeksv_amd/host/bam_reader.cpp seeksv_amd/host/bam_partition.cpp seeksv_amd/host/getsv_plan.cpp
HIP_SRC  = seeksv_amd/csrc/seeksv_hip.hip
# the `seeksv` command line: its sources, and the headers only they include
CLI_SRC  = seeksv_amd/host/seeksv_cli.cpp seeksv_amd/host/junction_stage.cpp seeksv_amd/host/readthrough_stage.cpp seeksv_amd/host/sam_text.cpp seeksv_amd/host/somatic_stage.cpp
CLI_DEPS = seeksv_amd/host/fastq_reads.h seeksv_amd/host/unmapped_pairs.h seeksv_amd/host/junction_stage.h seeksv_amd/host/readthrough_stage.h seeksv_amd/host/sam_text.h seeksv_amd/host/somatic_stage.h seeksv_amd/host/regions.h
HIP_DEPS = $(wildcard seeksv_amd/csrc/*.h) $(wildcard seeksv_amd/csrc/*.inc) $(wildcard seeksv_amd/csrc/*.hip) include/seeksv_hip.h

all: host hip synth cli primcheck

host: $(LIBDIR)/libseeksv_host.so
hip: $(LIBDIR)/libseeksv_hip.so
synth: $(LIBDIR)/libseeksv_synth.so $(LIBDIR)/libseeksv_synth_cpu.so
cli: seeksv_amd/bin/seeksv
primcheck: $(LIBDIR)/libseeksv_primcheck.so

$(LIBDIR)/libseeksv_host.so: $(HOST_SRC) $(wildcard seeksv_amd/host/*.h) include/seeksv_host.h include/seeksv_hip.h
	mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -lz -lpthread

$(LIBDIR)/libseeksv_hip.so: $(HIP_DEPS)
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(HIP_SRC)

# the `seeksv` command line (getclip / getsv) over the two libraries
seeksv_amd/bin/seeksv: $(CLI_SRC) $(CLI_DEPS) $(LIBDIR)/libseeksv_host.so $(LIBDIR)/libseeksv_hip.so
	mkdir -p seeksv_amd/bin
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude -o $@ $(CLI_SRC) -L$(LIBDIR) -lseeksv_host -lseeksv_hip -lz \
		-Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath-link,$(ROCM)/lib

# synthetic BAM-record generator: the same source compiled for the GPU (bench) and for the CPU (tests, cpu baseline)
$(LIBDIR)/libseeksv_synth.so: seeksv_amd/csrc/synth.hip seeksv_amd/csrc/synth_core.h
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ seeksv_amd/csrc/synth.hip

$(LIBDIR)/libseeksv_synth_cpu.so: seeksv_amd/csrc/synth_cpu.cpp seeksv_amd/csrc/synth_core.h
	mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -o $@ seeksv_amd/csrc/synth_cpu.cpp

# tests only: scan.h, radix_sort.h and tile_sort.h behind C entry points of their own (tests/test_primitives_gpu.py); not part of libseeksv_hip.so
$(LIBDIR)/libseeksv_primcheck.so: tests/native/prim_check.hip seeksv_amd/csrc/scan.h seeksv_amd/csrc/radix_sort.h seeksv_amd/csrc/tile_sort.h seeksv_amd/csrc/common.h
	mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Iseeksv_amd/csrc -shared -o $@ tests/native/prim_check.hip

oracle:
	$(MAKE) -C oracle liboracle.so

oracle-ref:
	$(MAKE) -C oracle ref

# Sanitizer pass over everything that runs on the CPU (GPU AddressSanitizer is not available on the pool): host library, CPU build of the
# generator, the oracle and the CLI's host stages under ASan + UBSan, then the CPU test suite against that build.
ASAN_DIR ?= /tmp/seeksv_asan
ASAN_FLAGS = -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined
asan: $(LIBDIR)/libseeksv_hip.so
	mkdir -p $(ASAN_DIR)
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -fPIC -Iinclude -shared -o $(ASAN_DIR)/libseeksv_host.so $(HOST_SRC) -lz -lpthread
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -fPIC -Iinclude -shared -o $(ASAN_DIR)/libseeksv_synth_cpu.so seeksv_amd/csrc/synth_cpu.cpp
	gcc $(ASAN_FLAGS) -std=c11 -Wall -Wextra -fPIC -shared -o $(ASAN_DIR)/liboracle.so oracle/seeksv_oracle.c -lm
	cp $(LIBDIR)/libseeksv_hip.so $(ASAN_DIR)/
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -Iinclude -o $(ASAN_DIR)/seeksv $(CLI_SRC) \
		-L$(ASAN_DIR) -lseeksv_host -lseeksv_hip -lz -Wl,-rpath,'$$ORIGIN' -Wl,-rpath-link,$(ROCM)/lib
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Iseeksv_amd/csrc tests/native/inflate_check.cpp -lz -o $(ASAN_DIR)/inflate_check && $(ASAN_DIR)/inflate_check
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -Iseeksv_amd/host tests/native/fastq_reads_check.cpp -o $(ASAN_DIR)/fastq_reads_check && $(ASAN_DIR)/fastq_reads_check
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -Iseeksv_amd/host tests/native/regions_check.cpp -lz -o $(ASAN_DIR)/regions_check && $(ASAN_DIR)/regions_check
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra tests/native/sa_parse_check.cpp -o $(ASAN_DIR)/sa_parse_check && $(ASAN_DIR)/sa_parse_check
	LD_PRELOAD=$$(gcc -print-file-name=libasan.so):$$(gcc -print-file-name=libubsan.so) ASAN_OPTIONS=detect_leaks=0:verify_asan_link_order=0 SSV_CLEAN_EXIT=1 \
		SSV_TEST_CXXFLAGS="$(ASAN_FLAGS)" SSV_LIBDIR=$(abspath $(ASAN_DIR)) SSV_ORACLE_SO=$(abspath $(ASAN_DIR))/liboracle.so SSV_CLI=$(abspath $(ASAN_DIR))/seeksv \
		python -m pytest tests -x -q -m "not gpu" -p no:cacheprovider

# The host rebuild of the cluster table's narrow wire form (seeksv_amd/csrc/table_wire.h, no HIP in it) as a program of its own under ASan + UBSan,
# against the encoder in the test program
wire-check:
	mkdir -p $(ASAN_DIR)
	$(CXX) $(ASAN_FLAGS) -std=c++17 -Wall -Wextra -Iseeksv_amd/csrc tests/native/table_wire_check.cpp -o $(ASAN_DIR)/table_wire_check && $(ASAN_DIR)/table_wire_check

clean:
	rm -rf $(LIBDIR) && $(MAKE) -C oracle clean

.PHONY: all host hip synth cli primcheck oracle oracle-ref asan wire-check clean
