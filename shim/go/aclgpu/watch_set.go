package aclgpu

/*
#include "shim.h"
*/
import "C"

import (
	"context"
	"sync"
	"time"
	"unsafe"

	"google.golang.org/grpc/codes"
	"google.golang.org/grpc/status"
)

// WatchSet binds acl_watch_set_t (include/aclgpu.h "watch sets"): the LookupResources rows of many watchers of one (resource type, permission)
// kept in device memory between polls.  A poll reports what every watcher gained or lost since its last answer, WHATEVER kind of write caused it --
// the reference's RunWatch (pkg/authz/watch.go:27-111) hears updates of the watched type only (watch.go:29-31) and misses a user put into a group, a
// nested group, a namespace grant and an expiring grant.  This differs from the reference on purpose and is OFF unless Config.WatchSets is set.
//
// ONE set is shared by all open watches of its shape, and a poll consumes the changes of ALL its watchers (it moves every watcher's baseline).  So a
// set has exactly one poll loop, Run, which hands every record to the sink of ITS watcher; the open watches register with Watch and never poll
// themselves.  poll is not exported and Run refuses to start twice: a second poller would silently eat the other watchers' changes.
type WatchSet struct {
	e      *Engine
	s      *C.acl_watch_set_t
	typeID C.int

	mu      sync.Mutex
	sinks   map[uint32]WatchSink
	running bool
	wake    chan struct{} // a watcher was added: poll now (its first answer does not wait for a write)
}

// WatchSink receives one watcher's changes, in (resource id) order per poll: allowed = gained.  It is called from the set's Run loop: it must not
// block for long (the patched RunWatch sends tracker.foundChanged <- resultChange{allowed, nn}, as watch.go:103-108 does per re-checked update).
type WatchSink func(allowed bool, objectID string)

// WatchChange is one acl_watch_change_t with the resource's name resolved (within the recycling quarantine, aclgpu.h).
type WatchChange struct {
	Watcher  uint32
	ObjectID string
	Allowed  bool // true: gained, false: lost -- resultChange.allowed of watch.go:21-24
	Wildcard bool // subject-direction sets: the record reports `subjectType:*` (ACL_WATCH_CHANGE_WILDCARD), not a concrete subject; ObjectID is "*"
}

// OpenWatchSet opens a set for subjects subjectType[#subjectRelation] against resourceType#permission.  Needs Config.WatchSets.
func (e *Engine) OpenWatchSet(resourceType, permission, subjectType, subjectRelation string) (*WatchSet, error) {
	if !e.watchSets {
		return nil, status.Error(codes.FailedPrecondition, "watch sets are switched off (Config.WatchSets): they report changes the reference's watch does not")
	}
	var cs cstrings
	defer cs.free()
	rt := C.acl_type_id(e.h, cs.add(resourceType))
	st := C.acl_type_id(e.h, cs.add(subjectType))
	pm := C.acl_relation_id(e.h, rt, cs.add(permission))
	sr := C.int(-1)
	if subjectRelation != "" && subjectRelation != "..." {
		if sr = C.acl_relation_id(e.h, st, cs.add(subjectRelation)); sr < 0 {
			sr = -2 // a relation that does not exist is not "no relation": FAILED_PRECONDITION from the engine
		}
	}
	w := &WatchSet{e: e, typeID: rt, sinks: map[uint32]WatchSink{}, wake: make(chan struct{}, 1)}
	if rc := C.acl_watch_set_open(e.h, rt, pm, st, sr, &w.s); rc != 0 {
		return nil, lastError(rc)
	}
	return w, nil
}

// OpenSubjectWatchSet opens a SUBJECT-direction set (acl_watch_set_open_subjects): the audit question.  Its watchers are resources of resourceType --
// Watch takes a resource id -- and its changes name the subjects of subjectType[#subjectRelation] that gained or lost permission on them: a
// WatchChange's ObjectID is a subject id, Wildcard marks the record of `subjectType:*`.  On a permission without `&` / `-` / `.all()` that a wildcard
// grants, the subjects behind the wildcard are not reported one by one.  Everything else -- one Run loop, Watch, Stats, Close -- is WatchSet's.
// Needs Config.WatchSets, as OpenWatchSet does: the reference has no counterpart.
func (e *Engine) OpenSubjectWatchSet(resourceType, permission, subjectType, subjectRelation string) (*WatchSet, error) {
	if !e.watchSets {
		return nil, status.Error(codes.FailedPrecondition, "watch sets are switched off (Config.WatchSets): they report changes the reference's watch does not")
	}
	var cs cstrings
	defer cs.free()
	rt := C.acl_type_id(e.h, cs.add(resourceType))
	st := C.acl_type_id(e.h, cs.add(subjectType))
	pm := C.acl_relation_id(e.h, rt, cs.add(permission))
	sr := C.int(-1)
	if subjectRelation != "" && subjectRelation != "..." {
		if sr = C.acl_relation_id(e.h, st, cs.add(subjectRelation)); sr < 0 {
			sr = -2
		}
	}
	w := &WatchSet{e: e, typeID: st, sinks: map[uint32]WatchSink{}, wake: make(chan struct{}, 1)} // (the records' ids are of the subject type)
	if rc := C.acl_watch_set_open_subjects(e.h, rt, pm, st, sr, &w.s); rc != 0 {
		return nil, lastError(rc)
	}
	return w, nil
}

// Watch registers one open watch: its changes go to sink from the next poll of Run on.  fromNow: the baseline is what the subject holds at that
// poll (nothing is reported for it: the watch follows an initial list); else it starts from the empty set, as the filter's allowedNames does
// (responsefilterer.go:509), and its first answer is everything it holds.  The returned func ends the watch (acl_watch_set_remove).
func (w *WatchSet) Watch(subjectID string, fromNow bool, sink WatchSink) (uint32, func() error, error) {
	var cs cstrings
	defer cs.free()
	var flags C.uint32_t
	if fromNow {
		flags = C.ACL_WATCHER_FROM_NOW
	}
	var id C.uint32_t
	w.mu.Lock() // (registered before the loop can poll the new watcher: no record without a sink)
	if rc := C.acl_watch_set_add(w.e.h, w.s, cs.add(subjectID), flags, &id); rc != 0 {
		w.mu.Unlock()
		return 0, nil, lastError(rc)
	}
	w.sinks[uint32(id)] = sink
	w.mu.Unlock()
	select {
	case w.wake <- struct{}{}:
	default:
	}
	stop := func() error {
		w.mu.Lock()
		defer w.mu.Unlock()
		delete(w.sinks, uint32(id))
		if rc := C.acl_watch_set_remove(w.e.h, w.s, id); rc != 0 {
			return lastError(rc)
		}
		return nil
	}
	return uint32(id), stop, nil
}

// poll walks every watcher on the current snapshot and returns the changes ordered by (watcher, resource id), the snapshot's revision and the raw
// return code.  A failed poll (a candidate's depth error under an exclusion, cancellation) leaves the baseline alone: the next one reports the whole
// difference.  Only Run calls it.
func (w *WatchSet) poll(ctx context.Context) ([]WatchChange, uint64, C.int, error) {
	opts, stop := callOpts(ctx)
	defer stop()
	var recs *C.acl_watch_change_t
	var n C.size_t
	var rev C.uint64_t
	if rc := C.acl_watch_set_poll(w.e.h, w.s, opts, &recs, &n, &rev); rc != 0 {
		return nil, 0, rc, status.Error(itemCode(C.int32_t(rc)), C.GoString(C.acl_last_error()))
	}
	if n == 0 {
		return nil, uint64(rev), 0, nil
	}
	defer C.acl_free(unsafe.Pointer(recs))
	out := make([]WatchChange, 0, int(n))
	buf := make([]C.char, 1025)
	for _, r := range unsafe.Slice(recs, int(n)) {
		ln := C.acl_object_name_copy(w.e.h, w.typeID, r.resource_id, &buf[0], C.size_t(len(buf)))
		if ln < 0 {
			continue // an anonymous (bulk-loaded) id: nothing the proxy could name
		}
		out = append(out, WatchChange{Watcher: uint32(r.watcher), ObjectID: C.GoStringN(&buf[0], C.int(ln)), Allowed: r.gained != 0, Wildcard: r.reserved&C.ACL_WATCH_CHANGE_WILDCARD != 0})
	}
	return out, uint64(rev), 0, nil
}

func (w *WatchSet) Stats() (polls, walks, changes uint64) {
	var p, k, c C.uint64_t
	C.acl_watch_set_stats(w.e.h, w.s, &p, &k, &c)
	return uint64(p), uint64(k), uint64(c)
}

// Close frees the set.  Run must have returned and no Watch / stop func may be in flight (acl_watch_set_close is exclusive, aclgpu.h).
func (w *WatchSet) Close() error {
	if rc := C.acl_watch_set_close(w.e.h, w.s); rc != 0 {
		return lastError(rc)
	}
	w.s = nil
	return nil
}

// Run is THE poll loop of the set -- RunWatch's loop (watch.go:37-110) for all its watchers at once: it blocks until ANY write is committed
// (acl_watch_wait over all types; every 200 ms it looks at ctx, and once a second it polls anyway -- an expiry arrives without a write) or a
// watcher is added, polls, and hands every change to the sink of its watcher.  It returns when ctx ends or the engine fails; a poll that fails
// with ACL_ERR_DEPTH (a candidate's confirming Check under an exclusion: the data may be mended by the next write) is retried after the next
// wake-up and loses nothing, the baseline having stayed.  Every other failure -- RESOURCE_EXHAUSTED included, which is permanent for a set whose
// difference has outgrown one poll -- ends the loop with the error.  A second Run on the same set is refused.
func (w *WatchSet) Run(ctx context.Context) error {
	w.mu.Lock()
	if w.running {
		w.mu.Unlock()
		return status.Error(codes.FailedPrecondition, "this watch set already has its poll loop: a second poller would consume the other watchers' changes")
	}
	w.running = true
	w.mu.Unlock()
	defer func() {
		w.mu.Lock()
		w.running = false
		w.mu.Unlock()
	}()
	var cursor C.uint64_t
	if rc := C.acl_watch_poll_go(w.e.h, C.uint64_t(^uint64(0)), nil, 0, nil, &cursor); rc != 0 {
		return lastError(rc)
	}
	for {
		changes, _, rc, err := w.poll(ctx)
		if err != nil && rc != C.ACL_ERR_DEPTH { // (the raw code: itemCode maps ACL_ERR_DEPTH onto ResourceExhausted, which a real one must not hide behind)
			return err
		}
		w.mu.Lock()
		for _, c := range changes {
			if sink := w.sinks[c.Watcher]; sink != nil { // (none: the watch ended between the poll and here)
				sink(c.Allowed, c.ObjectID)
			}
		}
		w.mu.Unlock()
		last := time.Now()
	wait:
		for {
			if err := ctx.Err(); err != nil {
				return status.FromContextError(err).Err()
			}
			select {
			case <-w.wake:
				break wait
			default:
			}
			opts := C.acl_call_opts_t{timeout_ns: C.int64_t(200 * time.Millisecond)}
			rc := C.acl_watch_wait(w.e.h, cursor, nil, 0, &opts, &cursor)
			if rc != 0 && rc != C.ACL_ERR_DEADLINE_EXCEEDED {
				return lastError(rc)
			}
			if rc == 0 || time.Since(last) > time.Second {
				break
			}
		}
	}
}
