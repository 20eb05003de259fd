/*
 * isg_rccl.inc -- the one cross-chain exchange of the sampler: every chain's stored log-likelihood samples
 * (CONVG.convg_ld, filled at mcmc.c:223-224) travel to every rank for the Gelman-Rubin check (check_converg.c:44-91).
 * The reference runs its chains back to back in one process (InStruct.c:182-193) and simply indexes one array; here each
 * chain is a process on its own GPU (instruct_amd/host/instruct_mgpu.c) and the samples are gathered with ONE
 * ncclAllGather over RCCL / xGMI on device buffers.  librccl is loaded on first use (a single-GPU run never touches it);
 * the ncclUniqueId goes from rank 0 to the others through a file in the launcher's rendezvous directory.
 */
#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>

struct RcclApi {
	void *h = nullptr;
	ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static int rccl_load(RcclApi &a)
{
	if (a.h) return 0;
	const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
	for (const char *n : names)
		if ((a.h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
	if (!a.h) return fail(std::string("isg_gather_convg: cannot load librccl: ") + dlerror());
	a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(a.h, "ncclGetUniqueId");
	a.CommInitRank = (decltype(a.CommInitRank))dlsym(a.h, "ncclCommInitRank");
	a.AllGather = (decltype(a.AllGather))dlsym(a.h, "ncclAllGather");
	a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.h, "ncclCommDestroy");
	a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.h, "ncclGetErrorString");
	if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) return fail("isg_gather_convg: librccl lacks an entry point");
	return 0;
}
#define NCCLCHK(x)                                                                                               \
	do {                                                                                                     \
		ncclResult_t r_ = (x);                                                                           \
		if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + api.GetErrorString(r_));             \
	} while (0)

extern "C" int isg_gather_convg(isg_ctx *c, int rank, int world, const char *id_path, const double *mine, int n, double *all)
{
	static RcclApi api;
	if (world < 1 || rank < 0 || rank >= world || n < 1) return fail("isg_gather_convg: bad rank / world / count");
	HIPCHK(hipSetDevice(c->cfg.device));
	if (rccl_load(api)) return 1;
	ncclUniqueId id;
	if (rank == 0) { /* published under a temporary name, then renamed: readers never see half of it */
		NCCLCHK(api.GetUniqueId(&id));
		const std::string tmp = std::string(id_path) + ".tmp";
		FILE *f = fopen(tmp.c_str(), "wb");
		if (!f || fwrite(&id, sizeof(id), 1, f) != 1) return fail("isg_gather_convg: cannot write the communicator id");
		fclose(f);
		if (rename(tmp.c_str(), id_path) != 0) return fail("isg_gather_convg: cannot publish the communicator id");
	} else {
		/* rank 0 publishes the id when ITS chain is done: the chains run the same number of iterations, so minutes apart at most (a chain
		 * that was discarded for an empty cluster and re-run, InStruct.c:185-190, takes twice as long: INSTRUCT_MGPU_TIMEOUT seconds,
		 * default half an hour).  The launcher leaves an `abort` file beside the id when a worker has failed: nobody waits for a dead rank. */
		const long limit_ms = 1000L * env_int(getenv("INSTRUCT_MGPU_TIMEOUT"), 1800L);
		std::string abort_path(id_path);
		const size_t slash = abort_path.find_last_of('/');
		abort_path = (slash == std::string::npos ? std::string("") : abort_path.substr(0, slash + 1)) + "abort";
		FILE *f = nullptr;
		for (long waited = 0; !(f = fopen(id_path, "rb")); waited += 20) {
			if (access(abort_path.c_str(), F_OK) == 0) return fail("isg_gather_convg: the launcher aborted the run (another worker failed)");
			if (waited > limit_ms) return fail("isg_gather_convg: timed out waiting for rank 0's communicator id");
			usleep(20000);
		}
		const size_t got = fread(&id, sizeof(id), 1, f);
		fclose(f);
		if (got != 1) return fail("isg_gather_convg: short communicator id file");
	}
	ncclComm_t comm;
	NCCLCHK(api.CommInitRank(&comm, world, id, rank));
	{ /* (the buffers go before the communicator, on every way out) */
		DevBuf<double> d_in, d_out;
		HIPCHK(d_in.alloc((size_t)n));
		HIPCHK(d_out.alloc((size_t)n * world));
		HIPCHK(hipMemcpyAsync(d_in, mine, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
		NCCLCHK(api.AllGather(d_in.get(), d_out.get(), (size_t)n, ncclDouble, comm, c->stream));
		HIPCHK(hipMemcpyAsync(all, d_out, sizeof(double) * (size_t)n * world, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	NCCLCHK(api.CommDestroy(comm));
	return 0;
}
