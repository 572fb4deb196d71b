package aclgpu

/*
#include "shim.h"
*/
import "C"

import (
	"errors"
	"unsafe"
)

// Sharded deployment (the north star's 8-GPU layout, SURVEY.md 8(e)): one process per GPU, each holding the rows of the
// object types with fnv1a(type) mod world == rank; the relationship store stays replicated (every rank applies every
// WriteRelationships).  The level loop runs INSIDE libaclgpu.so (acl_shard_check_bulk_rccl: one fixed-capacity
// ncclAllGather per dispatch level over xGMI, decisions on the device, one host synchronisation per burst of levels).
// UNBUILT here, like the rest of the shim.

// RcclUniqueID is made by rank 0 and handed to every rank by whatever channel the deployment has (the proxy replicas
// already share a control plane); it is the 128-byte ncclUniqueId.
func RcclUniqueID() ([C.ACL_RCCL_UNIQUE_ID_BYTES]byte, error) {
	var id [C.ACL_RCCL_UNIQUE_ID_BYTES]byte
	if rc := C.acl_shard_rccl_unique_id(unsafe.Pointer(&id[0])); rc != 0 {
		return id, lastError(rc)
	}
	return id, nil
}

// JoinShards turns this engine into shard `rank` of `world` and creates the library's RCCL communicator.
func (e *Engine) JoinShards(id [C.ACL_RCCL_UNIQUE_ID_BYTES]byte, rank, world uint32) error {
	if rc := C.acl_shard_rccl_init(e.h, unsafe.Pointer(&id[0]), C.uint32_t(rank), C.uint32_t(world)); rc != 0 {
		return lastError(rc)
	}
	return nil
}

// ShardedCheckBulk answers one batch with all shards together: SPMD, every rank calls it with the SAME interned batch
// (device pointers: the batch is uploaded once per rank by the caller, e.g. through hipMemcpy in a small C helper).
// perm / err come back identical on every rank.
func (e *Engine) ShardedCheckBulk(dItems unsafe.Pointer, n int, dPerm, dErr unsafe.Pointer) (levels, exchanges uint32, err error) {
	var st C.acl_shard_bulk_stats_t
	if rc := C.acl_shard_check_bulk_rccl(e.h, dItems, C.size_t(n), dPerm, dErr, &st); rc != 0 {
		return 0, 0, lastError(rc)
	}
	return uint32(st.levels), uint32(st.exchanges), nil
}

// ShardedLookupSubjects answers LookupSubjects for n resources of one (type, permission) with all shards together (acl_shard_subjects_bulk_rccl: the
// native level loop; the host-driven step protocol has no LookupSubjects).  SPMD: every rank calls it with the SAME interned ids.  dBitmaps (and
// dExcluded, which may be nil: not computed) are device pointers to n rows of bitmapWords words over the subject type's ids; flags[i] bit 0 says a
// `T:*` grant answers resource i (flags == nil: not wanted; a non-nil slice shorter than resourceIDs is an error).  Rows, flags and excluded rows come
// back identical on every rank; an error is returned by all ranks or by none.
func (e *Engine) ShardedLookupSubjects(rtype, permission, stype, srel int, resourceIDs []uint32, dBitmaps unsafe.Pointer, bitmapWords int, flags []uint8,
	dExcluded unsafe.Pointer) (levels, exchanges uint32, err error) {
	var st C.acl_shard_bulk_stats_t
	var ids *C.uint32_t
	if len(resourceIDs) > 0 {
		ids = (*C.uint32_t)(unsafe.Pointer(&resourceIDs[0]))
	}
	var fl *C.uint8_t
	if flags != nil && len(flags) < len(resourceIDs) {
		return 0, 0, errors.New("aclgpu: ShardedLookupSubjects: flags is shorter than resourceIDs")
	}
	if len(flags) > 0 {
		fl = (*C.uint8_t)(unsafe.Pointer(&flags[0]))
	}
	if rc := C.acl_shard_subjects_bulk_rccl(e.h, C.int(rtype), C.int(permission), C.int(stype), C.int(srel), ids, C.size_t(len(resourceIDs)), dBitmaps, C.size_t(bitmapWords), fl, dExcluded, &st); rc != 0 {
		return 0, 0, lastError(rc)
	}
	return uint32(st.levels), uint32(st.exchanges), nil
}
