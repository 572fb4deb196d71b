package aclgpu

/*
#include "shim.h"
*/
import "C"

import (
	"context"
	"encoding/base64"
	"io"
	"sort"
	"strconv"
	"strings"
	"sync"
	"time"

	v1 "github.com/authzed/authzed-go/proto/authzed/api/v1"
	"google.golang.org/grpc/codes"
	"google.golang.org/grpc/metadata"
	"google.golang.org/grpc/status"
)

// Paged LookupResources / LookupSubjects (optional_limit / optional_concrete_limit and optional_cursor): the engine's lookup cursors
// (aclgpu.h "paged lookups").  The first page opens a cursor -- ONE walk, the row stays on the device, pinned at that revision -- and every
// page after it is a few ids and their names out of that row, so all pages of one enumeration come from one snapshot, as SpiceDB's cursor
// pins the revision.  The engine wrapper keeps the open cursors in a small table:
//   - at most maxPagedCursors (64) at a time: opening one more closes the one used longest ago;
//   - a cursor not used for pagedCursorIdle (60 s) is closed the next time the table is touched (the reference abandons a prefilter after
//     10 s, responsefilterer.go:44; a kube client's `continue` token is good for minutes, which the idle time leans towards);
//   - a cursor whose row has been read to its end is closed at once.
// The token in AfterResultCursor is opaque: base64 of "key:row:last id".  An unknown or expired key answers FailedPrecondition ("start
// again"), as the engine itself answers for a cursor that a schema reload or a recycled object id has expired.
const (
	maxPagedCursors = 64
	pagedCursorIdle = 60 * time.Second
	pagedBlock      = 512 // names fetched per cgo call
)

type pagedCursor struct {
	mu      sync.Mutex // one page at a time per cursor; close waits for it
	cur     *C.acl_lookup_cursor_t
	request string // what the cursor answers: a token presented with another request is refused
	used    time.Time
	at      *v1.ZedToken
	empty   bool // an unknown resource (LookupSubjects): no rows, no pages
}

type cursorTable struct {
	mu   sync.Mutex
	next uint64
	open map[uint64]*pagedCursor
}

var pagedTables sync.Map // *Engine -> *cursorTable (the Engine struct stays as it is: the table exists only once a paged request arrives)

func (e *Engine) pagedTable() *cursorTable {
	t, _ := pagedTables.LoadOrStore(e, &cursorTable{open: map[uint64]*pagedCursor{}})
	return t.(*cursorTable)
}

func (e *Engine) closePaged(pc *pagedCursor) {
	pc.mu.Lock() // (a page in flight finishes first)
	defer pc.mu.Unlock()
	if pc.cur != nil {
		C.acl_lookup_cursor_close(e.h, pc.cur)
		pc.cur = nil
	}
}

// sweep drops idle cursors and, when the table is full, the one used longest ago.  Caller holds t.mu.
func (e *Engine) sweepPaged(t *cursorTable, makeRoom bool) {
	now := time.Now()
	var oldest uint64
	var oldestAt time.Time
	for k, pc := range t.open {
		if now.Sub(pc.used) > pagedCursorIdle {
			delete(t.open, k)
			go e.closePaged(pc)
			continue
		}
		if oldestAt.IsZero() || pc.used.Before(oldestAt) {
			oldest, oldestAt = k, pc.used
		}
	}
	if makeRoom && len(t.open) >= maxPagedCursors {
		pc := t.open[oldest]
		delete(t.open, oldest)
		go e.closePaged(pc)
	}
}

func (e *Engine) putPaged(pc *pagedCursor) uint64 {
	t := e.pagedTable()
	t.mu.Lock()
	defer t.mu.Unlock()
	e.sweepPaged(t, true)
	t.next++
	pc.used = time.Now()
	t.open[t.next] = pc
	return t.next
}

func (e *Engine) getPaged(key uint64, request string) (*pagedCursor, error) {
	t := e.pagedTable()
	t.mu.Lock()
	defer t.mu.Unlock()
	e.sweepPaged(t, false)
	pc, ok := t.open[key]
	if !ok {
		return nil, status.Error(codes.FailedPrecondition, "the cursor is unknown or has expired: start the enumeration again")
	}
	if pc.request != request {
		return nil, status.Error(codes.InvalidArgument, "the cursor belongs to another request")
	}
	pc.used = time.Now()
	return pc, nil
}

func (e *Engine) dropPaged(key uint64) {
	t := e.pagedTable()
	t.mu.Lock()
	pc, ok := t.open[key]
	delete(t.open, key)
	t.mu.Unlock()
	if ok {
		go e.closePaged(pc)
	}
}

func pagedToken(key uint64, row uint32, last uint32) *v1.Cursor {
	raw := strconv.FormatUint(key, 10) + ":" + strconv.FormatUint(uint64(row), 10) + ":" + strconv.FormatUint(uint64(last), 10)
	return &v1.Cursor{Token: base64.RawURLEncoding.EncodeToString([]byte(raw))}
}

func parsePagedToken(c *v1.Cursor) (key uint64, row uint32, last uint32, err error) {
	bad := status.Error(codes.FailedPrecondition, "the cursor is unknown or has expired: start the enumeration again")
	raw, derr := base64.RawURLEncoding.DecodeString(c.Token)
	if derr != nil {
		return 0, 0, 0, bad
	}
	parts := strings.Split(string(raw), ":")
	if len(parts) != 3 {
		return 0, 0, 0, bad
	}
	k, e1 := strconv.ParseUint(parts[0], 10, 64)
	r, e2 := strconv.ParseUint(parts[1], 10, 32)
	l, e3 := strconv.ParseUint(parts[2], 10, 32)
	if e1 != nil || e2 != nil || e3 != nil {
		return 0, 0, 0, bad
	}
	return k, uint32(r), uint32(l), nil
}

// pagedStream hands out up to `limit` names of one row (0: to the end of the row), a block per cgo call, each with the token that continues behind it
type pagedStream struct {
	ctx     context.Context
	e       *Engine
	pc      *pagedCursor
	key     uint64
	after   C.uint32_t // ACL_PAGE_FROM_START or the last id handed out
	left    uint32     // names still wanted; 0 with unlimited == true: no limit
	nolimit bool
	done    bool
	ids     []C.uint32_t
	ends    []C.uint32_t
	buf     []C.char
	n, k    int
}

// next: (name, token behind it) or io.EOF
func (s *pagedStream) next() (string, *v1.Cursor, error) {
	if err := s.ctx.Err(); err != nil {
		return "", nil, status.FromContextError(err).Err()
	}
	if s.k == s.n {
		if s.done || s.pc.empty || (!s.nolimit && s.left == 0) {
			return "", nil, io.EOF
		}
		if s.buf == nil {
			s.buf = make([]C.char, 64<<10)
			s.ends = make([]C.uint32_t, pagedBlock)
			s.ids = make([]C.uint32_t, pagedBlock)
		}
		want := uint32(pagedBlock)
		if !s.nolimit && s.left < want {
			want = s.left
		}
		var n C.uint32_t
		var more C.uint8_t
		s.pc.mu.Lock()
		if s.pc.cur == nil {
			s.pc.mu.Unlock()
			return "", nil, status.Error(codes.FailedPrecondition, "the cursor is unknown or has expired: start the enumeration again")
		}
		rc := C.acl_lookup_cursor_page_names(s.e.h, s.pc.cur, 0, s.after, C.uint32_t(want), &s.ids[0], &s.buf[0], C.size_t(len(s.buf)), &s.ends[0], &n, &more)
		s.pc.mu.Unlock()
		if rc != 0 {
			return "", nil, lastError(rc) // (FailedPrecondition: a schema reload or a recycled id expired the cursor -- "reopen")
		}
		s.n, s.k = int(n), 0
		if more == 0 {
			s.done = true
			s.e.dropPaged(s.key) // the row is read to its end: nothing left to continue
		}
		if n == 0 {
			return "", nil, io.EOF
		}
		if !s.nolimit {
			s.left -= uint32(n)
		}
	}
	from := 0
	if s.k > 0 {
		from = int(s.ends[s.k-1])
	}
	name := ""
	if end := int(s.ends[s.k]); end > from {
		name = C.GoStringN(&s.buf[from], C.int(end-from))
	}
	id := s.ids[s.k]
	s.after = id
	s.k++
	return name, pagedToken(s.key, 0, uint32(id)), nil
}

// openPaged: the cursor a paged request reads -- the one its token names, or a new one (one row: the request's subject or resource)
func (p *permissionsClient) openPaged(ctx context.Context, request string, token *v1.Cursor, limit uint32, open func(opts *C.acl_call_opts_t, out **C.acl_lookup_cursor_t) (C.int, bool)) (*pagedStream, error) {
	s := &pagedStream{ctx: ctx, e: p.e, after: C.ACL_PAGE_FROM_START, left: limit, nolimit: limit == 0}
	if token != nil {
		key, _, last, err := parsePagedToken(token)
		if err != nil {
			return nil, err
		}
		pc, err := p.e.getPaged(key, request)
		if err != nil {
			return nil, err
		}
		s.pc, s.key, s.after = pc, key, C.uint32_t(last)
		return s, nil
	}
	opts, stop := callOpts(ctx)
	defer stop()
	var cur *C.acl_lookup_cursor_t
	rc, empty := open(opts, &cur)
	if rc != 0 {
		return nil, status.Error(itemCode(C.int32_t(rc)), C.GoString(C.acl_last_error()))
	}
	pc := &pagedCursor{cur: cur, request: request, at: p.e.zedToken(), empty: empty}
	s.pc, s.key = pc, p.e.putPaged(pc)
	return s, nil
}

func (p *permissionsClient) lookupResourcesPaged(ctx context.Context, in *v1.LookupResourcesRequest) (v1.PermissionsService_LookupResourcesClient, error) {
	var cs cstrings
	defer cs.free()
	var st, sid, srel string
	if in.Subject != nil && in.Subject.Object != nil {
		st, sid, srel = in.Subject.Object.ObjectType, in.Subject.Object.ObjectId, in.Subject.OptionalRelation
	}
	request := "LR|" + in.ResourceObjectType + "|" + in.Permission + "|" + st + "|" + sid + "|" + srel
	s, err := p.openPaged(ctx, request, in.OptionalCursor, in.OptionalLimit, func(opts *C.acl_call_opts_t, out **C.acl_lookup_cursor_t) (C.int, bool) {
		rt := C.acl_type_id(p.e.h, cs.add(in.ResourceObjectType))
		stype := C.acl_type_id(p.e.h, cs.add(st))
		pm, sr := C.int(-1), C.int(-1)
		if rt >= 0 {
			pm = C.acl_relation_id(p.e.h, rt, cs.add(in.Permission))
		}
		if srel != "" && srel != "..." {
			sr = -2 // (a relation that does not exist is not "no relation")
			if stype >= 0 {
				if r := C.acl_relation_id(p.e.h, stype, cs.add(srel)); r >= 0 {
					sr = r
				}
			}
		}
		var subject C.uint32_t
		if stype >= 0 {
			// the subject's id: a subject nobody has a relationship with still holds what a `T:*` relationship grants
			if rc := C.acl_intern(p.e.h, stype, cs.add(sid), &subject); rc != 0 {
				return rc, false
			}
		}
		return C.acl_lookup_cursor_open(p.e.h, rt, pm, stype, sr, &subject, 1, opts, out), false
	})
	if err != nil {
		return nil, err
	}
	return &pagedResourceStream{s}, nil
}

type pagedResourceStream struct{ s *pagedStream }

func (r *pagedResourceStream) Recv() (*v1.LookupResourcesResponse, error) {
	name, token, err := r.s.next()
	if err != nil {
		return nil, err
	}
	return &v1.LookupResourcesResponse{LookedUpAt: r.s.pc.at, ResourceObjectId: name, AfterResultCursor: token,
		Permissionship: v1.LookupPermissionship_LOOKUP_PERMISSIONSHIP_HAS_PERMISSION}, nil
}
func (r *pagedResourceStream) Header() (metadata.MD, error) { return nil, nil }
func (r *pagedResourceStream) Trailer() metadata.MD         { return nil }
func (r *pagedResourceStream) CloseSend() error             { return nil }
func (r *pagedResourceStream) Context() context.Context     { return r.s.ctx }
func (r *pagedResourceStream) SendMsg(any) error            { return nil }
func (r *pagedResourceStream) RecvMsg(any) error            { return io.EOF }

func (p *permissionsClient) lookupSubjectsPaged(ctx context.Context, in *v1.LookupSubjectsRequest) (v1.PermissionsService_LookupSubjectsClient, error) {
	var cs cstrings
	defer cs.free()
	var rt, rid string
	if in.Resource != nil {
		rt, rid = in.Resource.ObjectType, in.Resource.ObjectId
	}
	request := "LS|" + rt + "|" + rid + "|" + in.Permission + "|" + in.SubjectObjectType + "|" + in.OptionalSubjectRelation
	wildcard := false
	s, err := p.openPaged(ctx, request, in.OptionalCursor, in.OptionalConcreteLimit, func(opts *C.acl_call_opts_t, out **C.acl_lookup_cursor_t) (C.int, bool) {
		rtype := C.acl_type_id(p.e.h, cs.add(rt))
		stype := C.acl_type_id(p.e.h, cs.add(in.SubjectObjectType))
		pm, sr := C.int(-1), C.int(-1)
		if rtype >= 0 {
			pm = C.acl_relation_id(p.e.h, rtype, cs.add(in.Permission))
		}
		if srel := in.OptionalSubjectRelation; srel != "" && srel != "..." {
			sr = -2
			if stype >= 0 {
				if r := C.acl_relation_id(p.e.h, stype, cs.add(srel)); r >= 0 {
					sr = r
				}
			}
		}
		var resource C.uint32_t
		n := C.size_t(1)
		if rtype < 0 || C.acl_find(p.e.h, rtype, cs.add(rid), &resource) != 0 {
			n = 0 // an unknown resource has no relationships: the empty answer (an unknown TYPE is refused by the open below)
		}
		rc := C.acl_lookup_cursor_open_subjects(p.e.h, rtype, pm, stype, sr, &resource, n, opts, out)
		if rc == 0 && n == 1 {
			var flag C.uint8_t
			if rc = C.acl_lookup_cursor_info(p.e.h, *out, nil, nil, nil, nil, &flag); rc == 0 && flag&C.ACL_SUBJECTS_WILDCARD != 0 {
				wildcard = true
			}
		}
		return rc, n == 0
	})
	if err != nil {
		return nil, err
	}
	if wildcard {
		// the subjects a wildcard leaves out are a row of their own that the engine does not page (aclgpu.h): refuse, do not answer half
		p.e.dropPaged(s.key)
		return nil, status.Error(codes.Unimplemented, "LookupSubjects with a limit over an answer that holds a wildcard is not implemented by the GPU ACL engine: ask without a limit")
	}
	return &pagedSubjectStream{s}, nil
}

type pagedSubjectStream struct{ s *pagedStream }

func (r *pagedSubjectStream) Recv() (*v1.LookupSubjectsResponse, error) {
	name, token, err := r.s.next()
	if err != nil {
		return nil, err
	}
	has := v1.LookupPermissionship_LOOKUP_PERMISSIONSHIP_HAS_PERMISSION
	return &v1.LookupSubjectsResponse{LookedUpAt: r.s.pc.at, SubjectObjectId: name, Permissionship: has, AfterResultCursor: token,
		Subject: &v1.ResolvedSubject{SubjectObjectId: name, Permissionship: has}}, nil
}
func (r *pagedSubjectStream) Header() (metadata.MD, error) { return nil, nil }
func (r *pagedSubjectStream) Trailer() metadata.MD         { return nil }
func (r *pagedSubjectStream) CloseSend() error             { return nil }
func (r *pagedSubjectStream) Context() context.Context     { return r.s.ctx }
func (r *pagedSubjectStream) SendMsg(any) error            { return nil }
func (r *pagedSubjectStream) RecvMsg(any) error            { return io.EOF }

// PrincipalSubject is one subject form of a kube principal: the user itself (`user:<name>`), or a group that authn attached to it, as the
// rule templates address it (`group:<name>#member`; rules.go:269).  Relation "" or "..." is no relation.
type PrincipalSubject struct{ Type, ID, Relation string }

// principalCursor binds the two calls of aclgpu.h "derived lookup cursors" for a pre-filter over `user` + `user.groups`: ONE
// acl_lookup_cursor_open_mixed over every subject form of every principal (one snapshot; the forms sorted by type and relation, so the engine
// walks once per form), then ONE acl_lookup_cursor_derive with an any-list per principal.  Row p of the cursor returned is what principal p
// may see: the union of its forms' individual answers -- the right definition for permissions with `-`, `&` and `.all()` too, which a
// reverse walk seeded with all the forms at once is not.  The mixed cursor is closed here; the caller pages the derived one
// (acl_lookup_cursor_page_names) and closes it.  No row crosses PCIe.
func (p *permissionsClient) principalCursor(ctx context.Context, resourceType, permission string, principals [][]PrincipalSubject) (*C.acl_lookup_cursor_t, error) {
	var cs cstrings
	defer cs.free()
	rt := C.acl_type_id(p.e.h, cs.add(resourceType))
	pm := C.int(-1)
	if rt >= 0 {
		pm = C.acl_relation_id(p.e.h, rt, cs.add(permission))
	}
	type flat struct {
		stype, srel C.int
		id          C.uint32_t
		principal   int
	}
	var all []flat
	for i, forms := range principals {
		for _, f := range forms {
			stype := C.acl_type_id(p.e.h, cs.add(f.Type))
			sr := C.int(-1)
			if f.Relation != "" && f.Relation != "..." {
				sr = -2 // (a relation that does not exist is not "no relation")
				if stype >= 0 {
					if r := C.acl_relation_id(p.e.h, stype, cs.add(f.Relation)); r >= 0 {
						sr = r
					}
				}
			}
			var id C.uint32_t
			if stype >= 0 {
				if rc := C.acl_intern(p.e.h, stype, cs.add(f.ID), &id); rc != 0 {
					return nil, lastError(rc)
				}
			}
			all = append(all, flat{stype, sr, id, i})
		}
	}
	sort.SliceStable(all, func(a, b int) bool {
		if all[a].stype != all[b].stype {
			return all[a].stype < all[b].stype
		}
		return all[a].srel < all[b].srel
	})
	subjects := make([]C.acl_subject_ref_t, len(all)+1) // (+1: &subjects[0] exists for a principal list without forms)
	perPrincipal := make([][]uint32, len(principals))
	for k, f := range all {
		subjects[k] = C.acl_subject_ref_t{stype: C.int32_t(f.stype), srel: C.int32_t(f.srel), id: f.id, reserved: 0}
		perPrincipal[f.principal] = append(perPrincipal[f.principal], uint32(k))
	}
	refs := make([]C.acl_row_ref_t, 0, len(all)+1)
	exprs := make([]C.acl_row_expr_t, len(principals)+1)
	for i, rows := range perPrincipal {
		if len(rows) == 0 {
			return nil, status.Error(codes.InvalidArgument, "a principal without a subject form")
		}
		exprs[i] = C.acl_row_expr_t{first: C.uint32_t(len(refs)), n_any: C.uint32_t(len(rows)), n_all: 0, n_none: 0}
		for _, row := range rows {
			refs = append(refs, C.acl_row_ref_t{cursor: 0, row: C.uint32_t(row)})
		}
	}
	refs = append(refs, C.acl_row_ref_t{cursor: 0, row: 0}) // (so that &refs[0] exists; not counted below)
	opts, stop := callOpts(ctx)
	defer stop()
	var mixed, derived *C.acl_lookup_cursor_t
	if rc := C.acl_lookup_cursor_open_mixed(p.e.h, rt, pm, &subjects[0], C.size_t(len(all)), opts, &mixed); rc != 0 {
		return nil, status.Error(itemCode(C.int32_t(rc)), C.GoString(C.acl_last_error()))
	}
	defer C.acl_lookup_cursor_close(p.e.h, mixed) // (the derived cursor owns its rows)
	if rc := C.acl_lookup_cursor_derive(p.e.h, &mixed, 1, &refs[0], C.size_t(len(refs)-1), &exprs[0], C.size_t(len(principals)), 0, &derived); rc != 0 {
		return nil, lastError(rc)
	}
	return derived, nil
}
