/*
 * emu_launch.h — the one launcher of the lane emulator (devport_emu.h): a workgroup's lanes as OS threads, a grid workgroup
 * after workgroup.  TEST INFRASTRUCTURE ONLY.  Every driver under tests/emu/ whose kernel body has a point where lanes meet
 * launches through it; the schedule-controlled mode of emu_lib.cpp creates its own, parked lanes.  The including translation
 * unit defines g_emu, once per library.
 */
#ifndef AACG_EMU_LAUNCH_H
#define AACG_EMU_LAUNCH_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "devport_emu.h"

enum { EMU_BLOCKS_FORWARD, EMU_BLOCKS_REVERSE };                 /* workgroups of a launch run in any order */

template <class Body> struct emu_lane_arg { emu_lane_ctx ctx; Body* body; };

template <class Body>
void* emu_lane_main(void* p)
{
    emu_lane_arg<Body>* a = (emu_lane_arg<Body>*)p;
    g_emu = a->ctx;
    (*a->body)();
    return nullptr;
}

/* one workgroup of `threads` lanes (a multiple of 64) with lds_bytes of LDS (0: none); body() runs once in every lane */
template <class Body>
void emu_launch_block(int block, int threads, size_t lds_bytes, Body& body)
{
    const int waves = threads / 64;
    std::vector<emu_wave> wv((size_t)waves);
    std::vector<emu_lane_arg<Body>> args((size_t)threads);
    std::vector<pthread_t> tid((size_t)threads);
    unsigned char* lds = lds_bytes ? (unsigned char*)aligned_alloc(512, (lds_bytes + 511) & ~(size_t)511) : nullptr;
    if (lds) std::memset(lds, 0xff, lds_bytes);                  /* NaN pattern: reads of unwritten LDS show up */
    emu_block blk;
    blk.lds = lds;
    blk.lds_bytes = lds_bytes;
    blk.block_id = block;
    blk.threads = threads; blk.sync_arrived = 0; blk.sync_gen = 0; blk.flags_off = -1;
    pthread_barrier_init(&blk.bar, nullptr, (unsigned)threads);
    for (int w = 0; w < waves; w++) { pthread_barrier_init(&wv[(size_t)w].bar, nullptr, 64); wv[(size_t)w].sw = nullptr; }
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 256 * 1024);
    for (int t = 0; t < threads; t++) {
        args[(size_t)t] = emu_lane_arg<Body>{emu_lane_ctx{t & 63, t >> 6, &wv[(size_t)(t >> 6)], &blk}, &body};
        if (pthread_create(&tid[(size_t)t], &attr, emu_lane_main<Body>, &args[(size_t)t])) { std::fprintf(stderr, "emu: cannot create lane thread %d\n", t); std::abort(); }
    }
    for (int t = 0; t < threads; t++) pthread_join(tid[(size_t)t], nullptr);
    for (int w = 0; w < waves; w++) pthread_barrier_destroy(&wv[(size_t)w].bar);
    pthread_barrier_destroy(&blk.bar);
    pthread_attr_destroy(&attr);
    free(lds);
}

/* a whole grid, workgroup after workgroup, in the given order */
template <class Body>
void emu_launch(int blocks, int threads, size_t lds_bytes, int order, Body body)
{
    for (int b = 0; b < blocks; b++) emu_launch_block(order == EMU_BLOCKS_REVERSE ? blocks - 1 - b : b, threads, lds_bytes, body);
}

#endif
