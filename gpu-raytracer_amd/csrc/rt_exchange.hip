// rt_exchange.hip -- the frame exchange of the tile split (rt_comm_*, rt_all_gather_*) of include/gpu_raytracer_amd.h.
#include <dlfcn.h>
#include "rt_context.h"

#include <cstdlib>
#include <cstring>

// ---- frame exchange of the tile split without Python ----------------------------------------------------
// One communicator per context. RCCL is bound at RUN TIME (dlopen, RTLD_LOCAL): a process that also hosts PyTorch already
// has torch's own copy of librccl mapped, and a link-time dependency would make every user of this library load a
// collective library most of them never call. Contexts that share a GPU (tests; RCCL refuses a device twice in one
// communicator) exchange by stream-ordered peer copies instead -- the same pack / unpack kernels either way.
namespace {
struct RcclUniqueId { char internal[128]; };            // ncclUniqueId (rccl.h)
enum { RCCL_FLOAT32 = 7 };                              // ncclFloat32
struct RcclApi {
	void * handle = nullptr;
	int (*get_unique_id)(RcclUniqueId *) = nullptr;
	int (*comm_init_rank)(void **, int, RcclUniqueId, int) = nullptr;
	int (*comm_init_all)(void **, int, const int *) = nullptr;
	int (*comm_destroy)(void *) = nullptr;
	int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
	int (*group_start)() = nullptr; int (*group_end)() = nullptr;
	const char * (*error_string)(int) = nullptr;
};
RcclApi * rccl_api(std::string & why) {
	static RcclApi api; static bool tried = false; static std::string failure;
	if (!tried) {
		tried = true;
		// GRT_COLLECTIVE_LIBRARY: another library with RCCL's entry points, tried first. tests/support/libloopback_ccl.so uses it to run this very code with two
		// ranks on a box with one GPU (RCCL refuses a device twice); a deployment could name a site's own RCCL build the same way.
		if (const char * named = getenv("GRT_COLLECTIVE_LIBRARY")) { if (named[0] && !(api.handle = dlopen(named, RTLD_NOW | RTLD_LOCAL))) failure = std::string("GRT_COLLECTIVE_LIBRARY: ") + dlerror(); }
		if (!api.handle && failure.empty()) for (const char * name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) if ((api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
		if (!api.handle) { if (failure.empty()) failure = std::string("librccl.so not found: ") + dlerror(); }
		else {
			#define RT_BIND(member, symbol) { *(void **)&api.member = dlsym(api.handle, symbol); if (!api.member) failure = std::string("librccl.so lacks ") + symbol; }
			RT_BIND(get_unique_id, "ncclGetUniqueId") RT_BIND(comm_init_rank, "ncclCommInitRank") RT_BIND(comm_init_all, "ncclCommInitAll") RT_BIND(comm_destroy, "ncclCommDestroy")
			RT_BIND(all_gather, "ncclAllGather") RT_BIND(group_start, "ncclGroupStart") RT_BIND(group_end, "ncclGroupEnd") RT_BIND(error_string, "ncclGetErrorString")
			#undef RT_BIND
		}
	}
	why = failure;
	return failure.empty() ? &api : nullptr;
}
// this rank's share of the frame in float4 pixels, padded so that every rank sends the same amount
size_t exchange_tiles_per_rank(const rt_context * ctx, int tile_pixels, int world) {
	size_t frame = size_t(ctx->params.screen_width) * ctx->params.screen_height;
	size_t tiles = (frame + tile_pixels - 1) / tile_pixels;
	return (tiles + world - 1) / world;
}
int exchange_buffers(rt_context * ctx, size_t pixels) {
	rt_context::FrameExchange & x = ctx->exchange;
	if (x.packed_pixels >= pixels) return RT_OK;
	if (x.packed)   device_free(ctx, x.packed);
	if (x.gathered) device_free(ctx, x.gathered);
	x.packed = x.gathered = nullptr; x.packed_pixels = 0;
	int status = device_alloc(ctx, (void **)&x.packed, pixels * 16); if (status) return status;
	status = device_alloc(ctx, (void **)&x.gathered, pixels * 16 * size_t(x.world)); if (status) return status;
	x.packed_pixels = pixels;
	if (!x.ev_packed) { RT_HIP(ctx, hipEventCreateWithFlags(&x.ev_packed, hipEventDisableTiming)); RT_HIP(ctx, hipEventCreateWithFlags(&x.ev_copied, hipEventDisableTiming)); }
	return RT_OK;
}
} // namespace

extern "C" {

int rt_comm_unique_id(void * out_id_128_bytes) {
	if (!out_id_128_bytes) return RT_ERROR_INVALID_ARG;
	std::string why; RcclApi * api = rccl_api(why);
	if (!api) return RT_ERROR_NOT_READY;
	return api->get_unique_id((RcclUniqueId *)out_id_128_bytes) == 0 ? RT_OK : RT_ERROR_HIP;
}

int rt_comm_init_rank(rt_context * ctx, const void * unique_id_128_bytes, int rank, int world) {
	RT_REQUIRE(ctx, ctx && unique_id_128_bytes && world >= 1 && rank >= 0 && rank < world, "rt_comm_init_rank: invalid argument");
	(void)hipSetDevice(ctx->device);
	(void)rt_comm_destroy(ctx);
	std::string why; RcclApi * api = rccl_api(why);
	if (!api) return fail(ctx, RT_ERROR_NOT_READY, "rt_comm_init_rank: %s", why.c_str());
	RcclUniqueId id; memcpy(&id, unique_id_128_bytes, sizeof(id));
	int rc = api->comm_init_rank(&ctx->exchange.comm, world, id, rank);
	if (rc != 0) { ctx->exchange.comm = nullptr; return fail(ctx, RT_ERROR_HIP, "rt_comm_init_rank: ncclCommInitRank: %s", api->error_string(rc)); }
	ctx->exchange.rank = rank; ctx->exchange.world = world;
	return RT_OK;
}

int rt_comm_init_all(rt_context ** contexts, int count) {
	if (!contexts || count < 1) return RT_ERROR_INVALID_ARG;
	for (int i = 0; i < count; i++) if (!contexts[i]) return RT_ERROR_INVALID_ARG;
	bool distinct = true;
	for (int i = 0; i < count; i++) for (int j = 0; j < i; j++) if (contexts[i]->device == contexts[j]->device) distinct = false;
	for (int i = 0; i < count; i++) { (void)rt_comm_destroy(contexts[i]); contexts[i]->exchange.rank = i; contexts[i]->exchange.world = count; }
	if (distinct && count > 1) {   // one communicator over the GPUs of this process (ncclCommInitAll)
		std::string why; RcclApi * api = rccl_api(why);
		if (!api) return fail(contexts[0], RT_ERROR_NOT_READY, "rt_comm_init_all: %s", why.c_str());
		std::vector<void *> comms(count, nullptr); std::vector<int> devices(count);
		for (int i = 0; i < count; i++) devices[i] = contexts[i]->device;
		int rc = api->comm_init_all(comms.data(), count, devices.data());
		if (rc != 0) return fail(contexts[0], RT_ERROR_HIP, "rt_comm_init_all: ncclCommInitAll: %s", api->error_string(rc));
		for (int i = 0; i < count; i++) contexts[i]->exchange.comm = comms[i];
	} else {                       // contexts sharing a GPU: stream-ordered copies between them
		for (int i = 0; i < count; i++) contexts[i]->exchange.peers.assign(contexts, contexts + count);
	}
	return RT_OK;
}

int rt_comm_destroy(rt_context * ctx) {
	if (!ctx) return RT_ERROR_INVALID_ARG;
	rt_context::FrameExchange & x = ctx->exchange;
	if (x.comm) { std::string why; if (RcclApi * api = rccl_api(why)) (void)api->comm_destroy(x.comm); x.comm = nullptr; }
	for (rt_context * peer : x.peers) if (peer && peer != ctx) {   // the others of an in-process group lose this member
		for (rt_context *& p : peer->exchange.peers) if (p == ctx) p = nullptr;
	}
	x.peers.clear();
	if (x.ev_packed || x.packed) {   // (a later group may have another world size: its buffers and events are made again, exchange_buffers)
		(void)hipSetDevice(ctx->device);
		(void)hipStreamSynchronize(ctx->stream);
	}
	if (x.ev_packed) { (void)hipEventDestroy(x.ev_packed); (void)hipEventDestroy(x.ev_copied); x.ev_packed = x.ev_copied = nullptr; }
	if (x.packed)   device_free(ctx, x.packed);
	if (x.gathered) device_free(ctx, x.gathered);
	x.packed = x.gathered = nullptr; x.packed_pixels = 0;
	x.rank = 0; x.world = 1;
	return RT_OK;
}

// what: 0 = the final image (1 float4 per pixel), 1 = the inputs of the SVGF filter stage (5 float4 per pixel)
static int exchange_group(rt_context ** contexts, int count, int what) {
	const int channels = what == 0 ? 1 : 5;
	std::string why; RcclApi * api = nullptr;
	// pack: every context's own tiles (the tile layout is the one rt_set_pixel_tiles gave it)
	for (int i = 0; i < count; i++) {
		rt_context * ctx = contexts[i];
		rt_context::FrameExchange & x = ctx->exchange;
		RT_REQUIRE(ctx, x.world == count || x.comm, "rt_all_gather: the contexts are not one communicator group");
		RT_REQUIRE(ctx, ctx->params.tile_pixels > 0 && ctx->params.tile_stride == x.world && ctx->params.tile_first == x.rank, "rt_all_gather: rt_set_pixel_tiles(tile_pixels, rank, world) first");
		(void)hipSetDevice(ctx->device);
		const size_t per_rank = exchange_tiles_per_rank(ctx, ctx->params.tile_pixels, x.world) * size_t(ctx->params.tile_pixels) * channels;
		int status = exchange_buffers(ctx, per_rank); if (status) return status;
		RT_HIP(ctx, main_waits_for_samples(ctx));
		if (!x.peers.empty()) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, x.ev_copied, 0));   // the peers have read the previous frame's tiles (see below)
		const int tiles = int(per_rank / size_t(ctx->params.tile_pixels) / channels);
		if (what == 0) rt_launch_pack_pixels(ctx->params, x.packed, ctx->params.tile_pixels, x.rank, x.world, tiles, ctx->stream);
		else { if (!ctx->svgf_allocated) return fail(ctx, RT_ERROR_NOT_READY, "rt_all_gather_svgf_inputs: SVGF is not enabled"); rt_launch_pack_svgf(slot_params(ctx, ctx->slots[0], 0), x.packed, ctx->params.tile_pixels, x.rank, x.world, tiles, ctx->stream); }
		RT_HIP(ctx, hipEventRecord(x.ev_packed, ctx->stream));
		if (x.comm && !api) { api = rccl_api(why); if (!api) return fail(ctx, RT_ERROR_NOT_READY, "rt_all_gather: %s", why.c_str()); }
	}
	// exchange
	if (api) {
		if (count > 1) api->group_start();
		for (int i = 0; i < count; i++) {
			rt_context * ctx = contexts[i]; rt_context::FrameExchange & x = ctx->exchange;
			(void)hipSetDevice(ctx->device);
			const size_t per_rank = exchange_tiles_per_rank(ctx, ctx->params.tile_pixels, x.world) * size_t(ctx->params.tile_pixels) * channels;
			int rc = api->all_gather(x.packed, x.gathered, per_rank * 4, RCCL_FLOAT32, x.comm, ctx->stream);
			if (rc != 0) { if (count > 1) api->group_end(); return fail(ctx, RT_ERROR_HIP, "rt_all_gather: ncclAllGather: %s", api->error_string(rc)); }
		}
		if (count > 1) { int rc = api->group_end(); if (rc != 0) return fail(contexts[0], RT_ERROR_HIP, "rt_all_gather: ncclGroupEnd: %s", api->error_string(rc)); }
	} else {
		for (int i = 0; i < count; i++) {
			rt_context * ctx = contexts[i]; rt_context::FrameExchange & x = ctx->exchange;
			RT_REQUIRE(ctx, int(x.peers.size()) == x.world && count == x.world, "rt_all_gather: an in-process group exchanges all its contexts in one call (rt_all_gather_framebuffers)");
			(void)hipSetDevice(ctx->device);
			const size_t per_rank = exchange_tiles_per_rank(ctx, ctx->params.tile_pixels, x.world) * size_t(ctx->params.tile_pixels) * channels;
			for (int r = 0; r < x.world; r++) {
				rt_context * peer = x.peers[r];
				RT_REQUIRE(ctx, peer && peer->exchange.packed_pixels >= per_rank, "rt_all_gather: a member of the group is gone");
				RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, peer->exchange.ev_packed, 0));
				if (peer->device == ctx->device) RT_HIP(ctx, hipMemcpyAsync(x.gathered + size_t(r) * per_rank, peer->exchange.packed, per_rank * 16, hipMemcpyDeviceToDevice, ctx->stream));
				else RT_HIP(ctx, hipMemcpyPeerAsync(x.gathered + size_t(r) * per_rank, ctx->device, peer->exchange.packed, peer->device, per_rank * 16, ctx->stream));
			}
		}
		// a context may pack its next frame only when every peer has copied this one: one event per context, recorded on a
		// stream that has waited for all the copies (its own stream does: the peers' copy streams are joined through ev_packed
		// of the NEXT round only, so join them here explicitly)
		for (int i = 0; i < count; i++) {
			rt_context * ctx = contexts[i];
			(void)hipSetDevice(ctx->device);
			RT_HIP(ctx, hipEventRecord(ctx->ev_interop, ctx->stream));
		}
		for (int i = 0; i < count; i++) {
			rt_context * ctx = contexts[i];
			(void)hipSetDevice(ctx->device);
			for (int r = 0; r < count; r++) if (r != i) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, contexts[r]->ev_interop, 0));
			RT_HIP(ctx, hipEventRecord(ctx->exchange.ev_copied, ctx->stream));
		}
	}
	// unpack: the gathered tiles become every context's whole frame
	for (int i = 0; i < count; i++) {
		rt_context * ctx = contexts[i]; rt_context::FrameExchange & x = ctx->exchange;
		(void)hipSetDevice(ctx->device);
		const int tiles = int(exchange_tiles_per_rank(ctx, ctx->params.tile_pixels, x.world));
		ctx->folds++;   // (other ranks' pixels replace this context's: a resolved image is older than the frame)
		if (what == 0) rt_launch_unpack_pixels(ctx->params, x.gathered, ctx->params.tile_pixels, x.world, tiles, ctx->stream);
		else rt_launch_unpack_svgf(slot_params(ctx, ctx->slots[0], 0), x.gathered, ctx->params.tile_pixels, x.world, tiles, ctx->stream);
		RT_HIP(ctx, hipGetLastError());
	}
	return RT_OK;
}

int rt_all_gather_framebuffer(rt_context * ctx) {
	RT_REQUIRE(ctx, ctx, "rt_all_gather_framebuffer: NULL context");
	if (ctx->exchange.world == 1 && !ctx->exchange.comm) return RT_OK;   // (a 1-rank communicator does run its ncclAllGather: tests/test_gpu_rccl.py)
	RT_REQUIRE(ctx, ctx->exchange.comm, "rt_all_gather_framebuffer: no communicator (rt_comm_init_rank), or an in-process group (use rt_all_gather_framebuffers)");
	return exchange_group(&ctx, 1, 0);
}
int rt_all_gather_framebuffers(rt_context ** contexts, int count) {
	if (!contexts || count < 1) return RT_ERROR_INVALID_ARG;
	if (count == 1 && contexts[0] && contexts[0]->exchange.world == 1) return RT_OK;
	return exchange_group(contexts, count, 0);
}
int rt_all_gather_svgf_inputs(rt_context ** contexts, int count) {
	if (!contexts || count < 1) return RT_ERROR_INVALID_ARG;
	if (count == 1 && contexts[0] && contexts[0]->exchange.world == 1) return RT_OK;
	return exchange_group(contexts, count, 1);
}

} // extern "C"
