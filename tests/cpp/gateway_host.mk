# TEST INFRASTRUCTURE: GatewayFlowSlot's host side (sentinel_amd/csrc/gateway_rules.h: rule validity, the conversion to
# ParamFlowRules and parser tables, gw_match) on the CPU, under the address and undefined-behaviour sanitizers (its own
# main, no GPU, no HIP; the sanitizer runtimes linked statically). Built in-tree by __graft_entry__.build(); run by
# tests/test_gateway_host.py and tests/test_gateway_abi.py.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
OUT   := $(ROOT)/build/tests

all: $(OUT)/test_gateway_host

$(OUT)/test_gateway_host: $(HERE)test_gateway_host.cpp $(ROOT)/sentinel_amd/csrc/gateway_rules.h \
                          $(ROOT)/include/sentinel_gpu.h
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
	    -static-libubsan -o $@ $<

.PHONY: all
